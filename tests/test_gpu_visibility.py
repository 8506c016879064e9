"""Sampled visibility on the device (include/srt_visibility.h; visibility.hip): a generator's S rays
from the surface point of every element, exported or traced in the same launch and counted.

Every comparison is exact -- rays on the uint32 view, `visible` bytes equal, `fraction` on the uint32
view -- against the host path (rtaRaysHost, rtaVisibilityHost), which tests/test_visibility_host.py
ties to a numpy restatement of DESIGN.md section 2 "Visibility" and to rtrOccludedHost. Scenes,
frames and generators are tests/visibility_cases.py's; a visibility test asserts its mix first.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import rays_cases as rc
import visibility_cases as vc
from scenefile import write_custom_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 3  # guard cells before and after every output


class Rig:
    """One scene on cuda:0, prepared at w x h; the calls return numpy arrays and check their guards."""

    def __init__(self, path, w, h):
        import torch

        import simpleraytracer_amd as srt

        self.torch = torch
        self.scene = srt.DeviceScene(path, 0)
        self.stream = torch.cuda.current_stream()
        self.scene.prepare(w, h, self.stream)
        self.w, self.h = w, h

    def up(self, a, dtype=f32):
        return self.torch.from_numpy(np.array(a, dtype)).cuda()  # (a copy: the shared cases are read-only)

    def _guarded(self, shape, dtype, fill):
        torch = self.torch
        count = int(np.prod(shape))
        item = count // shape[0] if shape[0] else 1
        flat = torch.full((count + 2 * GUARD * item,), fill, dtype=dtype, device="cuda")
        return flat, flat[GUARD * item:GUARD * item + count].view(*shape)

    def _check_guard(self, flat, inner, fill):
        lead = (flat.numel() - inner.numel()) // 2
        host = flat.cpu().numpy()
        edge = np.concatenate([host[:lead], host[host.size - lead:]])
        assert (edge == fill).all() if fill == fill else np.isnan(edge).all(), "a guard cell was written"

    def visibility(self, where, ids, gen, frame=False, row_begin=0, rows=None, want=("visible", "fraction")):
        """(visible, fraction) of a points call (where: positions) or a frame call (where: the band's
        offsets); a plane not in `want` is passed as None and comes back None."""
        torch = self.torch
        lead = (rows, self.w) if frame else (len(ids),)
        dw = self.up(where).reshape(*lead, 2)
        di = self.up(ids, np.int32).reshape(*lead)
        vflat, dv = self._guarded(lead, torch.uint8, 201)
        fflat, df = self._guarded(lead, torch.float32, float("nan"))
        g = vc.to_device(gen)
        kw = {"visible": dv if "visible" in want else None, "fraction": df if "fraction" in want else None}
        torch.cuda.synchronize()
        if frame:
            self.scene.visibility_frame(dw, di, g, row_begin=row_begin, row_count=rows, stream=self.stream, **kw)
        else:
            self.scene.visibility(dw, di, g, stream=self.stream, **kw)
        torch.cuda.synchronize()
        self._check_guard(vflat, dv, 201)
        self._check_guard(fflat, df, float("nan"))
        return dv.cpu().numpy().reshape(-1), df.cpu().numpy().reshape(-1)

    def rays(self, where, ids, gen, frame=False, row_begin=0, rows=None, keep=False):
        """(S, elements, 8) rays of generate_rays() / generate_rays_frame(); keep: the device tensor too."""
        torch = self.torch
        lead = (rows, self.w) if frame else (len(ids),)
        dw = self.up(where).reshape(*lead, 2)
        di = self.up(ids, np.int32).reshape(*lead)
        flat, dr = self._guarded((gen.count,) + lead + (8,), torch.float32, float("nan"))
        g = vc.to_device(gen)
        torch.cuda.synchronize()
        if frame:
            self.scene.generate_rays_frame(dw, di, g, dr, row_begin=row_begin, row_count=rows, stream=self.stream)
        else:
            self.scene.generate_rays(dw, di, g, dr, stream=self.stream)
        torch.cuda.synchronize()
        self._check_guard(flat, dr, float("nan"))
        out = dr.cpu().numpy().reshape(gen.count, -1, 8)
        return (out, dr) if keep else out

    def composed(self, where, ids, gen, **kw):
        """generate_rays -> scene.occluded -> count, on the device."""
        torch = self.torch
        _, dr = self.rays(where, ids, gen, keep=True, **kw)
        flat = dr.reshape(-1, 8)
        occ = torch.full((flat.shape[0],), 9, dtype=torch.uint8, device="cuda")
        self.scene.occluded(flat, occ, stream=self.stream)
        torch.cuda.synchronize()
        return (occ.reshape(gen.count, -1) == 0).sum(dim=0).to(torch.uint8).cpu().numpy()

    def stats(self, capfd):
        lines = re.findall(r"srt rays: scene \S+ builds (\d+) allocations (\d+)", capfd.readouterr().err)
        assert lines, "no ray counters on stderr: is SRT_SETUP_LOG honoured?"
        return tuple(int(v) for v in lines[-1])

    def close(self):
        self.scene.close()


def default_env(monkeypatch):
    monkeypatch.delenv("SRT_RAYS", raising=False)


def band_of(a, w, row_begin, rows):
    return np.asarray(a).reshape(-1, w, *np.shape(a)[1:])[row_begin:row_begin + rows].reshape(rows * w, *np.shape(a)[1:])


GENERATORS = {
    "hemisphere": lambda: vc.hemisphere(5, 0.3),
    "rotated": lambda: vc.hemisphere(5, 0.3, True),
    "area": lambda: vc.area_light(5),
    "mirror": vc.mirror,
}


@pytest.mark.parametrize("kind", list(GENERATORS))
@pytest.mark.parametrize("name,w,h,jitter", [("q", 48, 32, True), ("cornell", 70, 33, False), ("soup", 70, 33, True)])
def test_device_rays_equal_the_host(gpu, monkeypatch, name, w, h, jitter, kind):
    """G1: the whole frame, the band rows [5, 14) and points calls of 1, 257 and 2 240 elements."""
    default_env(monkeypatch)
    path = vc.scene_path(name)
    off, pos, ids = vc.frame_elements(name, w, h, jitter)
    gen = GENERATORS[kind]()
    turns = vc.frame_turns(w, h)
    want = vc.host_rays(path, w, h, pos, ids, gen, turns)
    assert (want[0, :, 4:7] != 0).any(axis=1).sum() >= 0.2 * len(ids), "too few elements on a surface"
    rig = Rig(path, w, h)
    vc.same_bits("frame rays", rig.rays(off, ids, gen, frame=True, rows=h), want)
    got = rig.rays(band_of(off.reshape(-1, 2), w, 5, 9), band_of(ids, w, 5, 9), gen, frame=True, row_begin=5, rows=9)
    vc.same_bits("band rays", got, want[:, 5 * w:14 * w])
    c = vc.points_case(name, w, h)
    reps = -(-2240 // len(c.ids))
    ppos, pids = np.tile(c.pos, (reps, 1))[:2240], np.tile(c.ids, reps)[:2240]
    pwant = vc.host_rays(path, w, h, ppos, pids, gen)
    for count in (1, 257, 2240):
        vc.same_bits(f"{count} points", rig.rays(ppos[:count], pids[:count], gen), pwant[:, :count])
    rig.close()


@pytest.mark.parametrize("mix", list(vc.MIXES))
@pytest.mark.parametrize("w,h,jitter", [(48, 32, False), (70, 33, True)])
def test_fused_equals_the_host_and_the_composition(gpu, monkeypatch, mix, w, h, jitter):
    """G2: visible and fraction of the whole frame, of the band rows [5, 14) and of a points call equal
    the host's, the device composition generate_rays -> occluded -> count, and both again under
    SRT_RAYS=brute."""
    default_env(monkeypatch)
    name, _ = vc.MIXES[mix]
    path = vc.scene_path(name)
    off, pos, ids = vc.frame_elements(name, w, h, jitter)
    gen, visible, fraction = vc.mix_answer(mix, w, h, jitter)
    S = gen.count
    vc.assert_mix(visible, ids, rc.vertices_of(path).shape[0], S)
    vc.same_bits("host fraction", fraction, vc.fraction_of(visible, S))
    boff, bids = band_of(off.reshape(-1, 2), w, 5, 9), band_of(ids, w, 5, 9)
    rig = Rig(path, w, h)
    for mode in ("tree", "brute"):
        if mode == "brute":
            monkeypatch.setenv("SRT_RAYS", "brute")
        v, f = rig.visibility(off, ids, gen, frame=True, rows=h)
        assert np.array_equal(v, visible), mode
        vc.same_bits(f"fraction ({mode})", f, fraction)
        assert np.array_equal(rig.composed(off, ids, gen, frame=True, rows=h), visible), mode
        v, f = rig.visibility(boff, bids, gen, frame=True, row_begin=5, rows=9)
        assert np.array_equal(v, visible[5 * w:14 * w]), mode
        vc.same_bits(f"band fraction ({mode})", f, fraction[5 * w:14 * w])
        v, f = rig.visibility(pos, ids, gen)  # (no rotation table: a points call is the frame's answer)
        assert np.array_equal(v, visible), mode
        vc.same_bits(f"points fraction ({mode})", f, fraction)
    monkeypatch.delenv("SRT_RAYS")
    rig.close()


@pytest.mark.parametrize("samples", [1, 7, 64])
def test_sample_counts(gpu, monkeypatch, samples):
    """G2: S = 1, 7 and 64 (the whole LDS table) on the soup's area light and Cornell's hemisphere."""
    default_env(monkeypatch)
    w, h = vc.FRAMES[0]
    for mix in ("soup_area", "cornell_hemisphere"):
        name, make = vc.MIXES[mix]
        path = vc.scene_path(name)
        off, pos, ids = vc.frame_elements(name, w, h, True)
        if samples == 64:
            pos, ids = pos[::4], ids[::4]
        gen = make(samples)
        visible, fraction = vc.host_visibility(path, w, h, pos, ids, gen)
        assert len(np.unique(visible[ids >= 0])) >= min(3, samples + 1)
        rig = Rig(path, w, h)
        v, f = rig.visibility(pos, ids, gen)
        assert np.array_equal(v, visible), mix
        vc.same_bits("fraction", f, fraction)
        assert np.array_equal(rig.composed(pos, ids, gen), visible), mix
        rig.close()


@pytest.mark.parametrize("n", [n for n in rc.COUNT_SOUPS if n != 0])
def test_triangle_counts_where_the_tree_changes_shape(gpu, monkeypatch, n):
    """G3: 400 points elements on soups of 1, 7, 8, 9, 63, 64, 65, 512, 513 and 4 097 triangles, a
    hemisphere and an area light."""
    from simpleraytracer_amd import device

    default_env(monkeypatch)
    w, h = vc.FRAMES[0]
    path = rc.soup_path(n)
    rng = np.random.default_rng(n)
    pos = rng.random((400, 2), dtype=f32)
    ids, _ = device.query_host(path, w, h, pos)
    # (a position that hits nothing takes a random triangle: the definition needs no hit, and every
    # tree is walked however few triangles are in view)
    ids = np.where(ids >= 0, ids, rng.integers(0, n, 400)).astype(np.int32)
    ids[::7] = -1
    ids[3::50] = n
    rig = Rig(path, w, h)
    for gen in (vc.hemisphere(8, 0.5), vc.area_light(8)):
        visible, fraction = device.visibility_host(path, w, h, pos, ids, gen)
        if n >= 512:
            assert (visible < 8).any(), "nothing is occluded"
        v, f = rig.visibility(pos, ids, gen)
        assert np.array_equal(v, visible)
        vc.same_bits("fraction", f, fraction)
    rig.close()


@pytest.mark.parametrize("mix,w,h", [("cornell_hemisphere", 70, 33), ("soup_hemisphere", 48, 32)])
def test_rotations(gpu, monkeypatch, mix, w, h):
    """G4: a random rotation table. A frame call indexes it by the pixel's place in its 4 x 4 block,
    with the absolute frame row in a band (row_begin = 5 is no multiple of 4); a points call by i & 15."""
    default_env(monkeypatch)
    name, _ = vc.MIXES[mix]
    path = vc.scene_path(name)
    off, pos, ids = vc.frame_elements(name, w, h, True)
    gen, visible, fraction = vc.mix_answer(mix, w, h, True, 8, True)
    plain = vc.mix_answer(mix, w, h, True)[1]
    vc.assert_mix(visible, ids, rc.vertices_of(path).shape[0], 8)
    assert (visible != plain).mean() >= 0.1, "the rotations change too little to be seen"
    rig = Rig(path, w, h)
    v, f = rig.visibility(off, ids, gen, frame=True, rows=h)
    assert np.array_equal(v, visible)
    vc.same_bits("fraction", f, fraction)
    v, f = rig.visibility(band_of(off.reshape(-1, 2), w, 5, 9), band_of(ids, w, 5, 9), gen, frame=True, row_begin=5, rows=9)
    assert np.array_equal(v, visible[5 * w:14 * w])
    vc.same_bits("band fraction", f, fraction[5 * w:14 * w])
    pv, pf = vc.host_visibility(path, w, h, pos, ids, gen)  # (i & 15)
    assert (pv != visible).any()
    v, f = rig.visibility(pos, ids, gen)
    assert np.array_equal(v, pv)
    vc.same_bits("points fraction", f, pf)
    rig.close()


def test_motion(gpu, monkeypatch, tmp_path, capfd):
    """G5: after set_vertices the fused answer is the host's on the moved file, with one more build of
    the tree and no new allocation; after set_camera it is the host's under the new camera, with no
    build at all."""
    from simpleraytracer_amd import device

    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    w, h = vc.FRAMES[0]
    path = vc.scene_path("soup")
    n = device.scene_triangles(path)
    gen = vc.hemisphere(8, 0.3)
    pos = device.pixel_positions(w, h, vc.offsets_of(w, h, True))

    def expect(file):
        ids, _ = device.query_host(file, w, h, pos)
        visible, fraction = device.visibility_host(file, w, h, pos, ids, gen)
        vc.assert_mix(visible, ids, n, 8)
        return ids, visible, fraction

    def check(file, builds):
        ids, visible, fraction = expect(file)
        v, f = rig.visibility(pos, ids, gen)
        assert np.array_equal(v, visible)
        vc.same_bits("fraction", f, fraction)
        assert rig.stats(capfd) == (builds, 1)

    rig = Rig(path, w, h)
    check(path, 1)
    v0 = rc.vertices_of(path)
    moved_v = (v0 + np.random.default_rng(9).uniform(-0.05, 0.05, v0.shape)).astype(f32)
    moved = write_custom_scene(tmp_path / "moved.srt", moved_v)
    rig.scene.set_vertices(rig.up(moved_v), stream=rig.stream)
    check(moved, 2)
    eye, lookat = (0.25, 0.125, -0.5), (0.0, 0.0, 3.0)
    turned = write_custom_scene(tmp_path / "turned.srt", moved_v, eye=eye, lookat=lookat)
    rig.scene.set_camera((*eye, *lookat, 0.0, 1.0, 0.0, 60.0), stream=rig.stream)
    check(turned, 2)
    rig.close()


def test_planes_and_edge_cases(gpu, monkeypatch):
    """G6: a plane left None is not written (its guard fill stays everywhere); no plane and zero
    counts enqueue nothing; the refusals reach the device forms; a scene never prepared is refused."""
    import ctypes

    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd import _native

    default_env(monkeypatch)
    w, h = vc.FRAMES[0]
    name, _ = vc.MIXES["soup_area"]
    path = vc.scene_path(name)
    off, pos, ids = vc.frame_elements(name, w, h, False)
    gen, visible, fraction = vc.mix_answer("soup_area", w, h, False)
    rig = Rig(path, w, h)
    v, f = rig.visibility(off, ids, gen, frame=True, rows=h, want=("visible",))
    assert np.array_equal(v, visible) and np.isnan(f).all()
    v, f = rig.visibility(pos, ids, gen, want=("fraction",))
    assert (v == 201).all()
    vc.same_bits("fraction", f, fraction)
    v, f = rig.visibility(pos, ids, gen, want=())
    assert (v == 201).all() and np.isnan(f).all()
    s, L = rig.scene, _native.lib()
    g = vc.to_device(gen)
    dpos, dids = rig.up(pos), rig.up(ids, np.int32)
    dv = torch.full((len(ids),), 201, dtype=torch.uint8, device="cuda")
    s.visibility(dpos[:0], dids[:0], g, visible=dv[:0])
    s.visibility_frame(rig.up(off)[:0], dids.reshape(h, w)[:0], g, visible=dv.reshape(h, w)[:0], row_begin=4, row_count=0)
    s.generate_rays(dpos[:0], dids[:0], g, torch.empty((8, 0, 8), device="cuda"))
    torch.cuda.synchronize()
    assert (dv.cpu().numpy() == 201).all()
    with pytest.raises(srt.SrtError, match="RTA_MIRROR"):
        s.visibility(dpos, dids, srt.Mirror(), visible=dv)
    with pytest.raises(srt.SrtError, match=r"rta_generator\.samples"):
        s.visibility(dpos, dids, srt.Hemisphere(torch.zeros((65, 3), device="cuda"), 0.0, 1.0), visible=dv)
    with pytest.raises(srt.SrtError, match=r"rta_generator\.eu"):
        s.visibility(dpos, dids, srt.AreaLight((0, 0, 0), (float("nan"), 0, 0), (0, 1, 0), g.samples), visible=dv)
    with pytest.raises(srt.SrtError, match="row band outside the frame"):
        s.visibility_frame(rig.up(off), dids.reshape(h, w), g, visible=dv.reshape(h, w), row_begin=1, row_count=h)
    with pytest.raises(ValueError, match="visible must be torch.uint8"):
        s.visibility(dpos, dids, g, visible=dv.float())
    with pytest.raises(ValueError, match="fraction must be"):
        s.visibility(dpos, dids, g, fraction=torch.empty(3, device="cuda"))
    with pytest.raises(ValueError, match="rays must be"):
        s.generate_rays(dpos, dids, g, torch.empty((len(ids), 8, 8), device="cuda"))
    with pytest.raises(ValueError, match="samples must be torch.float32"):
        s.visibility(dpos, dids, srt.AreaLight((0, 0, 0), (1, 0, 0), (0, 1, 0), g.samples.double()), visible=dv)
    gs = g._struct(lambda t: 0 if t is None else t.data_ptr())
    out = _native.RtaOutputs(ctypes.sizeof(_native.RtaOutputs), dv.data_ptr(), 0)
    assert L.rtaVisibilityPointsAsync(s.handle, None, dids.data_ptr(), 5, ctypes.byref(gs), ctypes.byref(out), None) == -1
    assert _native.last_error() == "Bad buffer argument: d_positions is NULL"
    assert L.rtaRaysPointsAsync(s.handle, dpos.data_ptr(), dids.data_ptr(), 5, ctypes.byref(gs), None, None) == -1
    assert _native.last_error() == "Bad buffer argument: d_rays is NULL"
    rig.close()
    bare = srt.DeviceScene(path, 0)
    with pytest.raises(srt.SrtError, match="Prepare"):
        bare.visibility(dpos, dids, g, visible=dv)
    bare.close()
