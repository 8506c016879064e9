"""G-buffer outputs on the device (include/srt_gbuffer.h rtgFrameAsync / rtgPointsAsync; outputs.hip
GBufferKernel): depth, barycentrics, normal + shading cosine and albedo + id from hit ids.

Expected values come from the oracle and numpy (tests/gbuffer_cases.py), never from the library:
depth, barycentrics and albedo are compared on the uint32 view, the normal within 2^-22 with its
sign, and albedo.rgb * normal.w, albedo.a on the uint32 view against the RGBA frame srtTraceAsync
stores for the same offsets.

Frames are 200 x 150 -- 4 x 10 tiles of 64 x 16, the last column and row partial -- unless a test
says otherwise; scene Q and the position families are tests/query_cases.py's.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import gbuffer_cases as gc
import query_cases as qc

pytestmark = pytest.mark.gpu

W, H = qc.W, qc.H
W2, H2 = 333, 170
PAD = 64             # elements past every output plane
SENTINEL = -77777.0  # no attribute takes this value: depth > 0 or +inf, |w| and |n| small, alpha >= -1
PLANES = (("depth", ()), ("bary", (2,)), ("normal", (4,)), ("albedo", (4,)))


@pytest.fixture(scope="module")
def scene_q(tmp_path_factory):
    return qc.write_scene_q(tmp_path_factory.mktemp("gbuffer") / "q.srt")


class Rig:
    """One scene on cuda:0 and its stream. gbuffer() and attributes() allocate every plane asked
    for PAD elements longer, prefilled with SENTINEL, check that the tail is untouched and the
    body fully written, and return the bodies as numpy arrays."""

    def __init__(self, path, w=None, h=None):
        import torch

        import simpleraytracer_amd as srt

        self.torch = torch
        self.scene = srt.DeviceScene(path, 0)
        self.stream = torch.cuda.current_stream()
        if w is not None:
            self.prepare(w, h)

    def prepare(self, w, h):
        self.w, self.h = w, h
        self.scene.prepare(w, h, self.stream)

    def dev(self, a, dtype):
        return self.torch.from_numpy(np.array(a, dtype)).cuda()  # (a copy: the shared cases are read-only)

    def query(self, pos):
        torch = self.torch
        n = len(pos)
        ids = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        t = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        self.scene.query(self.dev(pos, np.float32), ids, t, stream=self.stream)
        torch.cuda.synchronize()
        return ids.cpu().numpy(), t.cpu().numpy()

    def trace(self, offsets, ids=False):
        torch = self.torch
        off = self.dev(offsets, np.float32)
        if ids:
            out = torch.full((self.h, self.w), -7, dtype=torch.int32, device="cuda")
            self.scene.trace_ids(off, out, stream=self.stream)
        else:
            out = torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda")
            self.scene.trace(off, out, stream=self.stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def _planes(self, lead, which):
        torch = self.torch
        count = int(np.prod(lead))
        raw, views = {}, {}
        for name, tail in PLANES:
            if name in which:
                ch = int(np.prod(tail)) if tail else 1
                raw[name] = torch.full(((count + PAD) * ch,), SENTINEL, dtype=torch.float32, device="cuda")
                views[name] = raw[name][:count * ch].view(lead + tail)
        return raw, views

    def _collect(self, lead, raw, views):
        self.torch.cuda.synchronize()
        out = {}
        for name, v in views.items():
            body = v.cpu().numpy()
            tail = raw[name][body.size:].cpu().numpy()
            assert tail.size >= PAD and np.all(tail == np.float32(SENTINEL)), f"{name}: written past its end"
            assert not np.any(body == np.float32(SENTINEL)), f"{name}: not fully written"
            out[name] = body
        return out

    def gbuffer(self, offsets, ids, r0=0, rows=None, which=("depth", "bary", "normal", "albedo"), stream=None):
        rows = self.h - r0 if rows is None else rows
        off = self.dev(offsets[r0:r0 + rows], np.float32)
        idv = self.dev(ids[r0:r0 + rows], np.int32)
        raw, views = self._planes((rows, self.w), which)
        self.torch.cuda.synchronize()
        self.scene.gbuffer(off, idv, row_begin=r0, row_count=rows, stream=self.stream if stream is None else stream,
                           **views)
        return self._collect((rows, self.w), raw, views)

    def attributes(self, pos, ids, which=("depth", "bary", "normal", "albedo"), stream=None):
        raw, views = self._planes((len(pos),), which)
        p, i = self.dev(pos, np.float32), self.dev(ids, np.int32)
        self.torch.cuda.synchronize()
        self.scene.attributes(p, i, stream=self.stream if stream is None else stream, **views)
        return self._collect((len(pos),), raw, views)

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


@pytest.fixture(scope="module")
def frame_q(gpu, scene_q):
    """The whole-frame G-buffer of scene Q with random offsets (seed 3) from the trace's ids, the
    ids and the traced RGBA: computed once, read-only."""
    off = qc.random_offsets(W, H, 3)
    rig = Rig(scene_q, W, H)
    ids = rig.trace(off, ids=True)
    rgba = rig.trace(off)
    planes = rig.gbuffer(off, ids)
    rig.close()
    for a in (off, ids, rgba, *planes.values()):
        a.setflags(write=False)
    return off, ids, rgba, planes


def test_whole_frame(scene_q, frame_q, monkeypatch):
    default_env(monkeypatch)
    off, ids, rgba, g = frame_q
    pos, want_ids, exp = gc.cached_expected(scene_q, W, H, "pixels")
    qc.assert_mix(want_ids)
    assert np.array_equal(ids.reshape(-1), want_ids)
    assert g["depth"].shape == (H, W) and g["bary"].shape == (H, W, 2) and g["normal"].shape == (H, W, 4)
    gc.check_planes(exp, **g)
    gc.check_misses(ids, exp.n, exp.background, **g)
    gc.check_identity(g["normal"], g["albedo"], rgba)
    gc.check_shade(scene_q, W, H, off, ids, g["normal"], g["albedo"])
    hit = exp.valid
    assert (exp.cos64[hit] > 0).sum() >= 1000 and (exp.cos64[hit] < 0).sum() >= 1000  # both signs of the flip


def test_band(scene_q, frame_q, monkeypatch):
    """Rows 40..117: not tile-aligned; band-local buffers; every plane the slice of the whole frame's."""
    default_env(monkeypatch)
    off, ids, _, g = frame_q
    rig = Rig(scene_q, W, H)
    band = rig.gbuffer(off, ids, r0=40, rows=78)
    rig.close()
    same(band, {k: v[40:118] for k, v in g.items()})


def test_points(scene_q, frame_q, monkeypatch):
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    off, ids, _, g = frame_q
    pos, want_ids, exp = gc.cached_expected(scene_q, W, H, "mixed")
    qc.assert_mix(want_ids)
    rig = Rig(scene_q, W, H)
    q_ids, q_t = rig.query(pos)
    a = rig.attributes(pos, q_ids)
    pixels = device.pixel_positions(W, H, off)
    b = rig.attributes(pixels, ids.reshape(-1))
    rig.close()
    assert np.array_equal(q_ids, want_ids)
    gc.check_planes(exp, **a)
    gc.check_misses(q_ids, exp.n, exp.background, **a)
    assert np.array_equal(a["depth"].view(np.uint32), q_t.view(np.uint32))  # the query's own t
    same(b, {k: v.reshape((H * W,) + v.shape[2:]) for k, v in g.items()})


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_bounds_counts(scene_q, frame_q, monkeypatch, count):
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    off, ids, _, g = frame_q
    first = 75 * W + 60  # mid-frame: hits and misses among the first 257
    pixels = device.pixel_positions(W, H, off)[first:first + count]
    sub = ids.reshape(-1)[first:first + count]
    rig = Rig(scene_q, W, H)
    a = rig.attributes(pixels, sub)  # (the rig checks the padded tail and the body)
    rig.close()
    same(a, {k: v.reshape((H * W,) + v.shape[2:])[first:first + count] for k, v in g.items()})


@pytest.mark.parametrize("w,h", [(1, 1), (65, 17)])
def test_bounds_frames(scene_q, monkeypatch, w, h):
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    off = qc.random_offsets(w, h, 4)
    rig = Rig(scene_q, w, h)
    ids = rig.trace(off, ids=True)
    rgba = rig.trace(off)
    g = rig.gbuffer(off, ids)
    rig.close()
    assert w == 1 or ((ids >= 0).any() and (ids < 0).any())
    exp = gc.expected(scene_q, w, h, device.pixel_positions(w, h, off), ids.reshape(-1))
    gc.check_planes(exp, **g)
    gc.check_identity(g["normal"], g["albedo"], rgba)


def test_invalid_ids(scene_q, frame_q, monkeypatch):
    """Ids outside the scene scattered among valid ones: the miss values; the neighbours unaffected."""
    default_env(monkeypatch)
    off, ids, _, g = frame_q
    _, _, exp = gc.cached_expected(scene_q, W, H, "pixels")
    bad = gc.miss_ids(exp.n)
    mixed = ids.copy()
    flat = mixed.reshape(-1)
    at = np.random.default_rng(8).choice(flat.size, 50, replace=False)
    flat[at] = np.resize(bad, at.size)
    rig = Rig(scene_q, W, H)
    a = rig.gbuffer(off, mixed)
    rig.close()
    gc.check_misses(mixed, exp.n, exp.background, **a)
    keep = np.ones(flat.size, bool)
    keep[at] = False
    for name, v in a.items():
        got = v.reshape((flat.size,) + v.shape[2:])
        want = g[name].reshape(got.shape)
        assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32)), name


def test_optional_planes(scene_q, frame_q, monkeypatch):
    """Each plane alone gives the bits of all four together; no plane at all succeeds."""
    default_env(monkeypatch)
    off, ids, _, g = frame_q
    pos, q_ids, _ = gc.cached_expected(scene_q, W, H, "mixed")
    rig = Rig(scene_q, W, H)
    every = rig.attributes(pos, q_ids)
    for name, _ in PLANES:
        one = rig.gbuffer(off, ids, which=(name,))
        same(one, {name: g[name]})
        one = rig.attributes(pos, q_ids, which=(name,))
        same(one, {name: every[name]})
    pair = rig.gbuffer(off, ids, which=("normal", "albedo"))
    same(pair, {k: g[k] for k in ("normal", "albedo")})
    assert rig.gbuffer(off, ids, which=()) == {} and rig.attributes(pos, q_ids, which=()) == {}
    rig.close()


def test_no_setup(scene_q, monkeypatch, capfd):
    """The G-buffer builds and reads no cull setup: none before it, one after a trace, same bits."""
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    pos, want_ids, exp = gc.cached_expected(scene_q, W, H, "mixed")
    ids, _ = device.query_host(scene_q, W, H, pos)
    rig = Rig(scene_q, W, H)
    before = rig.attributes(pos, ids)
    builds_before = rig.stats(capfd)[0]
    rig.trace(qc.random_offsets(W, H, 3))
    builds_traced = rig.stats(capfd)[0]
    after = rig.attributes(pos, ids)
    builds_after = rig.stats(capfd)[0]
    rig.close()
    assert (builds_before, builds_traced, builds_after) == (0, 1, 1)
    gc.check_planes(exp, **before)
    same(before, after)


def test_reprepare_on_a_second_stream(scene_q, frame_q, monkeypatch):
    """prepare(333, 170), a trace on the first stream, the G-buffer on a second right after, no host
    sync in between: the values follow the new frame."""
    import torch

    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    off2 = qc.random_offsets(W2, H2, 6)
    pixels = device.pixel_positions(W2, H2, off2)
    want_ids, _ = device.query_host(scene_q, W2, H2, pixels)
    sel = np.random.default_rng(1).choice(W2 * H2, 3000, replace=False)  # the oracle's share of the frame
    exp = gc.expected(scene_q, W2, H2, pixels[sel], want_ids[sel])
    rig = Rig(scene_q, W, H)
    rig.gbuffer(frame_q[0], frame_q[1])
    rig.prepare(W2, H2)
    other = torch.cuda.Stream()
    off_d = rig.dev(off2, np.float32)
    ids_d = torch.full((H2, W2), -7, dtype=torch.int32, device="cuda")
    raw, views = rig._planes((H2, W2), [n for n, _ in PLANES])
    torch.cuda.synchronize()
    rig.scene.trace_ids(off_d, ids_d, stream=rig.stream)
    rig.scene.gbuffer(off_d, ids_d, stream=other, **views)  # reads the ids the trace is still writing
    g = rig._collect((H2, W2), raw, views)
    ids = ids_d.cpu().numpy()
    rgba = rig.trace(off2)
    rig.close()
    assert np.array_equal(ids.reshape(-1), want_ids)
    picked = {k: v.reshape((H2 * W2,) + v.shape[2:])[sel] for k, v in g.items()}
    gc.check_planes(exp, **picked)
    gc.check_identity(g["normal"], g["albedo"], rgba)


def test_long_scene(scenes, monkeypatch):
    """soup-100k at 1920 x 1080: band rows 536..539 with the trace's ids, 4 096 random points with the
    query's; depth against the oracle's full scan, and the RGBA identity."""
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    w, h = 1920, 1080
    path = scenes["soup100k"]
    rng = np.random.default_rng(17)
    off = np.full((h, w, 2), 0.5, np.float32)
    points = rng.random((4096, 2), dtype=np.float32)
    pixels = device.pixel_positions(w, h, 0.5).reshape(h, w, 2)[536:540, :1024].reshape(-1, 2)
    want_ids, want_t = qc.oracle_answers(path, w, h, np.concatenate([points, pixels]))
    assert (want_ids >= 0).sum() >= 0.10 * len(want_ids) and (want_ids < 0).sum() >= 0.10 * len(want_ids)
    rig = Rig(path, w, h)
    ids = rig.trace(off, ids=True)
    rgba = rig.trace(off)
    band = rig.gbuffer(off, ids, r0=536, rows=4)
    q_ids, q_t = rig.query(points)
    pts = rig.attributes(points, q_ids)
    rig.close()
    qc.assert_same(q_ids, pts["depth"], want_ids[:4096], want_t[:4096])
    qc.assert_same(ids[536:540, :1024].reshape(-1), band["depth"][:, :1024].reshape(-1), want_ids[4096:], want_t[4096:])
    gc.check_identity(band["normal"], band["albedo"], rgba[536:540])
    assert np.array_equal(pts["albedo"][:, 3], q_ids.astype(np.float32))


def test_errors(scene_q, monkeypatch):
    import ctypes

    import torch

    from simpleraytracer_amd import SrtError, _native

    default_env(monkeypatch)
    L = _native.lib()
    f32 = dict(dtype=torch.float32, device="cuda")
    rig = Rig(scene_q)
    pos = torch.full((4, 2), 0.5, **f32)
    pid = torch.zeros((4,), dtype=torch.int32, device="cuda")
    depth = torch.zeros((4,), **f32)
    # a scene that was never prepared
    with pytest.raises(SrtError, match=r"GBuffer: Prepare\(\) has not been called"):
        rig.scene.attributes(pos, pid, depth=depth)
    rig.prepare(W, H)
    off = torch.full((H, W, 2), 0.5, **f32)
    ids = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    fdepth = torch.zeros((H, W), **f32)
    out = _native.RtgOutputs(ctypes.sizeof(_native.RtgOutputs), depth.data_ptr(), 0, 0, 0)
    fout = _native.RtgOutputs(ctypes.sizeof(_native.RtgOutputs), fdepth.data_ptr(), 0, 0, 0)
    h = rig.scene.handle
    # NULL scene, NULL outputs, wrong struct_size
    assert L.rtgPointsAsync(None, pos.data_ptr(), pid.data_ptr(), 4, ctypes.byref(out), None) == -1
    assert _native.last_error() == "Bad scene handle"
    assert L.rtgFrameAsync(None, off.data_ptr(), ids.data_ptr(), 0, H, ctypes.byref(fout), None) == -1
    assert L.rtgPointsAsync(h, pos.data_ptr(), pid.data_ptr(), 4, None, None) == -1
    for size in (0, 32, 48):
        wrong = _native.RtgOutputs(size, depth.data_ptr(), 0, 0, 0)
        assert L.rtgPointsAsync(h, pos.data_ptr(), pid.data_ptr(), 4, ctypes.byref(wrong), None) == -1
        assert "struct_size" in _native.last_error()
        assert L.rtgFrameAsync(h, off.data_ptr(), ids.data_ptr(), 0, H, ctypes.byref(wrong), None) == -1
    # NULL inputs with a nonzero count; nothing to do with a zero count or no plane
    assert L.rtgPointsAsync(h, None, pid.data_ptr(), 4, ctypes.byref(out), None) == -1
    assert "d_positions" in _native.last_error()
    assert L.rtgPointsAsync(h, pos.data_ptr(), None, 4, ctypes.byref(out), None) == -1
    assert "d_ids" in _native.last_error()
    assert L.rtgFrameAsync(h, None, ids.data_ptr(), 0, H, ctypes.byref(fout), None) == -1
    assert "d_offsets" in _native.last_error()
    assert L.rtgFrameAsync(h, off.data_ptr(), None, 0, H, ctypes.byref(fout), None) == -1
    assert "d_ids" in _native.last_error()
    none = _native.RtgOutputs(ctypes.sizeof(_native.RtgOutputs), 0, 0, 0, 0)
    assert L.rtgPointsAsync(h, None, None, 0, ctypes.byref(out), None) == 0
    assert L.rtgFrameAsync(h, None, None, 0, 0, ctypes.byref(fout), None) == 0
    assert L.rtgPointsAsync(h, None, None, 4, ctypes.byref(none), None) == 0
    assert L.rtgFrameAsync(h, None, None, 0, H, ctypes.byref(none), None) == 0
    # a band past the frame
    assert L.rtgFrameAsync(h, off.data_ptr(), ids.data_ptr(), 1, H, ctypes.byref(fout), None) == -1
    assert "outside the frame" in _native.last_error()
    assert L.rtgFrameAsync(h, off.data_ptr(), ids.data_ptr(), H + 1, 0, ctypes.byref(fout), None) == -1
    with pytest.raises(SrtError, match="outside the frame"):
        rig.scene.gbuffer(off[:10], ids[:10], depth=fdepth[:10], row_begin=H - 5, row_count=10)
    # the wrapper's shape / dtype / device checks
    with pytest.raises(ValueError):
        rig.scene.attributes(torch.zeros((4, 3), **f32), pid, depth=depth)
    with pytest.raises(ValueError):
        rig.scene.attributes(pos, torch.zeros((5,), dtype=torch.int32, device="cuda"), depth=depth)
    with pytest.raises(ValueError):
        rig.scene.attributes(pos, pid.to(torch.int64), depth=depth)
    with pytest.raises(ValueError):
        rig.scene.attributes(pos, pid, depth=torch.zeros((5,), **f32))
    with pytest.raises(ValueError):
        rig.scene.attributes(pos, pid, bary=torch.zeros((4, 3), **f32))
    with pytest.raises(ValueError):
        rig.scene.attributes(pos, pid, normal=torch.zeros((4, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        rig.scene.attributes(pos.cpu(), pid, depth=depth)
    with pytest.raises(ValueError):
        rig.scene.gbuffer(off, ids, depth=torch.zeros((H, W, 1), **f32))
    with pytest.raises(ValueError):
        rig.scene.gbuffer(off[:, :-1], ids, depth=fdepth)
    with pytest.raises(ValueError):
        rig.scene.gbuffer(off, ids, albedo=torch.zeros((H, W, 4), **f32).cpu())
    # a valid call still works afterwards
    pos_np = np.full((4, 2), 0.5, np.float32)
    want_ids, want_t = qc.oracle_answers(scene_q, W, H, pos_np)
    got = rig.attributes(pos_np, want_ids, which=("depth",))
    rig.close()
    qc.assert_same(want_ids, got["depth"], want_ids, want_t)
