"""Multi-sample frames on the device (include/srt_samples.h rtsResolveAsync / rtsRenderAsync;
outputs.hip ResolveKernel): S hit-id planes and S sample-offset planes in, one resolved RGBA pixel out.

Expected values come from S per-sample RGBA frames -- srtTraceAsync's, or the oracle's -- resolved in
numpy (tests/samples_cases.py expected()), never from the resolve under test: bit-equal on the
uint32 view to the resolve of the traced frames and to rtsResolveHost, coverage exact and rgb within
1e-5 + S * 2^-24 against the oracle.

Scene S on cuda:0; frames are 200 x 150 -- 4 x 10 tiles of 64 x 16, the last column and row partial,
one block and a partial block of 256 pixels per row -- unless a test says otherwise. Every output is
allocated 64 elements longer and prefilled with a sentinel: the tail must stay untouched and the
body be fully written.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import query_cases as qc
import samples_cases as sc

pytestmark = pytest.mark.gpu

W, H, S = qc.W, qc.H, 5
W2, H2, S2 = 333, 170, 9
PAD = 64             # elements past every output
SENTINEL = -77777.0  # no resolved value: rgb >= 0, 0 <= alpha <= 1; no id either


@pytest.fixture(scope="module")
def scene_s(tmp_path_factory):
    return sc.write_scene_s(tmp_path_factory.mktemp("samples") / "s.srt")


class Rig:
    """One scene on cuda:0 and its stream. Outputs are allocated PAD elements longer, prefilled
    with SENTINEL, and checked: tail untouched, body fully written; returned as numpy arrays."""

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

    def planes(self, arrays, dtype):
        return [self.dev(a, dtype) for a in arrays]

    def padded(self, shape, dtype, fill):
        count = int(np.prod(shape))
        raw = self.torch.full((count + PAD,), fill, dtype=dtype, device="cuda")
        return raw, raw[:count].view(shape)

    def collect(self, raw, view, fill):
        self.torch.cuda.synchronize()
        body = view.cpu().numpy()
        tail = raw[body.size:].cpu().numpy()
        assert tail.size == PAD and np.all(tail == fill), "written past its end"
        assert not np.any(body == fill), "not fully written"
        return body

    def resolve(self, off, ids, r0=0, rows=None, stream=None):
        rows = self.h - r0 if rows is None else rows
        offs = self.planes([o[r0:r0 + rows] for o in off], np.float32)
        idp = self.planes([i[r0:r0 + rows] for i in ids], np.int32)
        raw, rgba = self.padded((rows, self.w, 4), self.torch.float32, SENTINEL)
        self.torch.cuda.synchronize()
        self.scene.resolve(offs, idp, rgba, row_begin=r0, row_count=rows, stream=self.stream if stream is None else stream)
        return self.collect(raw, rgba, np.float32(SENTINEL))

    def render_samples(self, off, variant="cull"):
        """(rgba (H, W, 4), ids (S, H, W)) of render_samples, the id planes padded and checked too."""
        offs = self.planes(off, np.float32)
        id_bufs = [self.padded((self.h, self.w), self.torch.int32, int(SENTINEL)) for _ in off]
        raw, rgba = self.padded((self.h, self.w, 4), self.torch.float32, SENTINEL)
        self.torch.cuda.synchronize()
        self.scene.render_samples(offs, [v for _, v in id_bufs], rgba, variant=variant, stream=self.stream)
        out = self.collect(raw, rgba, np.float32(SENTINEL))
        return out, np.stack([self.collect(r, v, int(SENTINEL)) for r, v in id_bufs])

    def trace(self, off, ids=False):
        """Every sample plane traced on its own: (S, H, W) ids, or (S, H, W, 4) RGBA."""
        torch = self.torch
        out = []
        for o in off:
            o_d = self.dev(o, np.float32)
            if ids:
                buf = torch.full((self.h, self.w), -7, dtype=torch.int32, device="cuda")
                self.scene.trace_ids(o_d, buf, stream=self.stream)
            else:
                buf = torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda")
                self.scene.trace(o_d, buf, stream=self.stream)
            torch.cuda.synchronize()
            out.append(buf.cpu().numpy())
        return np.stack(out)

    def shade(self, off, ids):
        torch = self.torch
        rgba = torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda")
        self.scene.shade(self.dev(off, np.float32), self.dev(ids, np.int32), rgba, stream=self.stream)
        torch.cuda.synchronize()
        return rgba.cpu().numpy()

    def stats(self, capfd):
        lines = re.findall(r"srt setup: scene \S+ builds (\d+) shared_frames (\d+) per_frame_frames (\d+)",
                           capfd.readouterr().err)
        assert lines, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
        return tuple(int(v) for v in lines[-1])

    def close(self):
        self.scene.close()


def default_env(monkeypatch):
    for name in ("SRT_SETUP", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_TRACE_RECORDS", "SRT_SETUP_LOG",
                 "SRT_CULL_CHUNKS", "SRT_CULL_SPLIT"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def frame_s(gpu, scene_s):
    """200 x 150, S = 5: the offsets, the traced id planes, the traced RGBA frames and the resolve
    of the id planes; computed once, read-only."""
    off = sc.offsets(W, H, S)
    rig = Rig(scene_s, W, H)
    ids = rig.trace(off, ids=True)
    frames = rig.trace(off)
    resolved = rig.resolve(off, ids)
    rig.close()
    for a in (off, ids, frames, resolved):
        a.setflags(write=False)
    return off, ids, frames, resolved


def test_identity(scene_s, frame_s, monkeypatch):
    """Bit-equal to the numpy resolve of srtTraceAsync's five frames and to rtsResolveHost; within
    1.03e-5 of the oracle (observed: 0, on the device as on the host)."""
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    off, ids, frames, resolved = frame_s
    o_off, o_frames, o_ids, n = sc.oracle_frames(scene_s, W, H, S)
    sc.assert_conditions(o_ids, n)
    assert np.array_equal(off, o_off) and np.array_equal(ids, o_ids)
    assert resolved.shape == (H, W, 4)
    sc.same_bits("resolve vs the traced frames", resolved, sc.expected(frames))
    sc.same_bits("resolve vs resolve_host", resolved, device.resolve_host(scene_s, W, H, off, ids))
    sc.check_against_oracle("resolve 200x150 S=5", resolved, o_frames)


@pytest.mark.parametrize("samples", [1, 2, 7, 8, 9, 15, 16])
def test_render_samples(scene_s, monkeypatch, samples):
    """render_samples: the bits of separate trace_ids + resolve, its id planes the oracle's. 9, 15 and
    16 cross the 8-frame trace batch; 9 leaves a remainder for every sample group size. The kernel
    takes S < 8 in groups of 4 and S >= 8 in groups of 8, what is left in halving groups: 7 is 4 + 2 +
    1 on the one side of that threshold, 8 and 15 = 8 + 4 + 2 + 1 on the other."""
    default_env(monkeypatch)
    off, o_frames, o_ids, n = sc.oracle_frames(scene_s, W, H, samples)
    if samples >= S:
        sc.assert_conditions(o_ids, n)
    rig = Rig(scene_s, W, H)
    rgba, ids = rig.render_samples(off)
    separate = rig.resolve(off, rig.trace(off, ids=True))
    rig.close()
    assert np.array_equal(ids, o_ids)
    sc.same_bits("render_samples vs trace_ids + resolve", rgba, separate)
    sc.check_against_oracle(f"render_samples S={samples}", rgba, o_frames)


def test_render_samples_other_variant(scene_s, frame_s, monkeypatch):
    """A variant that is traced frame by frame gives the same planes and pixels."""
    default_env(monkeypatch)
    off, ids, _, resolved = frame_s
    rig = Rig(scene_s, W, H)
    rgba, got_ids = rig.render_samples(off, variant="lds")
    rig.close()
    assert np.array_equal(got_ids, ids)
    sc.same_bits("render_samples(lds)", rgba, resolved)


def test_setup_counters(scene_s, frame_s, monkeypatch, capfd):
    """A bare resolve builds no cull setup; render_samples at S = 9 builds one for its two batches."""
    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    off, ids, _, resolved = frame_s
    off9 = sc.offsets(W, H, S2)
    rig = Rig(scene_s, W, H)
    bare = rig.resolve(off, ids)
    after_resolve = rig.stats(capfd)
    rig.render_samples(off9)
    after_render = rig.stats(capfd)
    rig.close()
    assert after_resolve == (0, 0, 0)
    assert after_render == (1, S2, 0)
    sc.same_bits("resolve on a fresh frame", bare, resolved)


def test_band(scene_s, frame_s, monkeypatch):
    """Rows 40..117: not tile-aligned; band-local buffers; the slice of the whole frame."""
    default_env(monkeypatch)
    off, ids, _, resolved = frame_s
    r0, rows = sc.BAND
    rig = Rig(scene_s, W, H)
    band = rig.resolve(off, ids, r0=r0, rows=rows)
    rig.close()
    sc.same_bits("band 40..117", band, resolved[r0:r0 + rows])


@pytest.mark.parametrize("w,h", [(1, 1), (65, 17)])
def test_small_frames(scene_s, monkeypatch, w, h):
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    off, o_frames, o_ids, n = sc.oracle_frames(scene_s, w, h, S)
    if w > 1:
        sc.assert_conditions(o_ids, n)
    rig = Rig(scene_s, w, h)
    ids = rig.trace(off, ids=True)
    frames = rig.trace(off)
    got = rig.resolve(off, ids)
    rendered, r_ids = rig.render_samples(off)
    rig.close()
    assert np.array_equal(ids, o_ids) and np.array_equal(r_ids, o_ids)
    sc.same_bits("resolve vs the traced frames", got, sc.expected(frames))
    sc.same_bits("resolve vs resolve_host", got, device.resolve_host(scene_s, w, h, off, ids))
    sc.same_bits("render_samples", rendered, got)
    sc.check_against_oracle(f"resolve {w}x{h} S=5", got, o_frames)


def test_one_sample_and_four_copies(scene_s, frame_s, monkeypatch):
    """S = 1, and the same plane two and four times: rgb bit-equal to shade()'s; alpha is the coverage."""
    default_env(monkeypatch)
    off, ids, frames, _ = frame_s
    rig = Rig(scene_s, W, H)
    shaded = rig.shade(off[2], ids[2])
    one = rig.resolve([off[2]], [ids[2]])
    two = rig.resolve([off[2]] * 2, [ids[2]] * 2)
    four = rig.resolve([off[2]] * 4, [ids[2]] * 4)
    rig.close()
    sc.same_bits("shade() vs the traced frame", shaded, frames[2])
    sc.same_bits("S = 1", one[..., :3], shaded[..., :3])
    assert np.array_equal(one[..., 3], (ids[2] >= 0).astype(np.float32))
    sc.same_bits("two copies", two, one)
    sc.same_bits("four copies", four, one)


def test_out_of_range_ids(scene_s, frame_s, monkeypatch):
    """Ids outside the scene over 50 samples that hit: those samples are misses, every other
    pixel keeps its bits."""
    default_env(monkeypatch)
    off, ids, frames, resolved = frame_s
    n = sc.oracle_frames(scene_s, W, H, S)[3]
    mixed, at = sc.scatter_misses(ids, n)
    rig = Rig(scene_s, W, H)
    got = rig.resolve(off, mixed)
    rig.close()
    sc.same_bits("out-of-range ids", got, sc.expected(sc.frames_with_misses(frames, at, sc.BACKGROUND)))
    touched = np.zeros(H * W, bool)
    touched[at % (H * W)] = True
    assert np.all(got.reshape(-1, 4)[touched, 3] < resolved.reshape(-1, 4)[touched, 3])
    sc.same_bits("the other pixels", got.reshape(-1, 4)[~touched], resolved.reshape(-1, 4)[~touched])


def test_resolve_on_a_second_stream(scene_s, frame_s, monkeypatch):
    """prepare(333, 170), the nine id planes traced in two batches on the first stream, the resolve
    on a second right after, no host synchronisation in between: the synchronous answer."""
    import torch

    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    off, o_frames, o_ids, n = sc.oracle_frames(scene_s, W2, H2, S2)
    sc.assert_conditions(o_ids, n)
    rig = Rig(scene_s, W, H)
    rig.resolve(frame_s[0], frame_s[1])
    rig.prepare(W2, H2)
    other = torch.cuda.Stream()
    offs = rig.planes(off, np.float32)
    idp = [torch.full((H2, W2), -7, dtype=torch.int32, device="cuda") for _ in range(S2)]
    raw, rgba = rig.padded((H2, W2, 4), torch.float32, SENTINEL)
    torch.cuda.synchronize()
    rig.scene.trace_batch(offs[:8], idp[:8], ids=True, stream=rig.stream)
    rig.scene.trace_batch(offs[8:], idp[8:], ids=True, stream=rig.stream)
    rig.scene.resolve(offs, idp, rgba, stream=other)  # reads the ids the traces are still writing
    got = rig.collect(raw, rgba, np.float32(SENTINEL))
    ids = np.stack([i.cpu().numpy() for i in idp])
    again = rig.resolve(off, ids)
    rig.close()
    assert np.array_equal(ids, o_ids)
    sc.same_bits("second stream vs synchronous", got, again)
    sc.same_bits("second stream vs resolve_host", got, device.resolve_host(scene_s, W2, H2, off, ids))
    sc.check_against_oracle("resolve 333x170 S=9", got, o_frames)


def test_errors(scene_s, frame_s, monkeypatch):
    import ctypes

    import torch

    from simpleraytracer_amd import SrtError, _native

    default_env(monkeypatch)
    L = _native.lib()
    f32 = dict(dtype=torch.float32, device="cuda")
    rig = Rig(scene_s)
    off = [torch.full((H, W, 2), 0.5, **f32) for _ in range(2)]
    ids = [torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(2)]
    rgba = torch.zeros((H, W, 4), **f32)
    arr = ctypes.c_void_p * 2
    offs, idp = arr(*[o.data_ptr() for o in off]), arr(*[i.data_ptr() for i in ids])
    h = rig.scene.handle
    # a scene that was never prepared
    assert L.rtsResolveAsync(h, offs, idp, 2, 0, 0, rgba.data_ptr(), None) == -1
    assert "Prepare() has not been called" in _native.last_error()
    assert L.rtsRenderAsync(h, offs, idp, 2, rgba.data_ptr(), _native.SRT_TRACE_CULL, None) == -1
    assert "Prepare() has not been called" in _native.last_error()
    rig.prepare(W, H)
    # NULL scene
    assert L.rtsResolveAsync(None, offs, idp, 2, 0, H, rgba.data_ptr(), None) == -1
    assert _native.last_error() == "Bad scene handle"
    assert L.rtsRenderAsync(None, offs, idp, 2, rgba.data_ptr(), _native.SRT_TRACE_CULL, None) == -1
    assert _native.last_error() == "Bad scene handle"
    # samples
    for bad in (0, _native.RTS_MAX_SAMPLES + 1):
        assert L.rtsResolveAsync(h, offs, idp, bad, 0, H, rgba.data_ptr(), None) == -1
        assert "samples" in _native.last_error()
        assert L.rtsRenderAsync(h, offs, idp, bad, rgba.data_ptr(), _native.SRT_TRACE_CULL, None) == -1
        assert "samples" in _native.last_error()
    # NULL arrays, NULL entries, NULL output
    assert L.rtsResolveAsync(h, None, idp, 2, 0, H, rgba.data_ptr(), None) == -1
    assert "d_offsets is NULL" in _native.last_error()
    assert L.rtsResolveAsync(h, offs, None, 2, 0, H, rgba.data_ptr(), None) == -1
    assert "d_ids is NULL" in _native.last_error()
    assert L.rtsResolveAsync(h, arr(off[0].data_ptr(), None), idp, 2, 0, H, rgba.data_ptr(), None) == -1
    assert "d_offsets[1]" in _native.last_error()
    assert L.rtsResolveAsync(h, offs, arr(None, ids[1].data_ptr()), 2, 0, H, rgba.data_ptr(), None) == -1
    assert "d_ids[0]" in _native.last_error()
    assert L.rtsResolveAsync(h, offs, idp, 2, 0, H, None, None) == -1
    assert "d_rgba" in _native.last_error()
    assert L.rtsRenderAsync(h, None, idp, 2, rgba.data_ptr(), _native.SRT_TRACE_CULL, None) == -1
    assert "d_offsets is NULL" in _native.last_error()
    assert L.rtsRenderAsync(h, offs, arr(ids[0].data_ptr(), None), 2, rgba.data_ptr(), _native.SRT_TRACE_CULL, None) == -1
    assert "d_ids[1]" in _native.last_error()
    assert L.rtsRenderAsync(h, offs, idp, 2, None, _native.SRT_TRACE_CULL, None) == -1
    assert "d_rgba" in _native.last_error()
    assert L.rtsRenderAsync(h, offs, idp, 2, rgba.data_ptr(), 99, None) == -1
    assert "variant" in _native.last_error()
    # a band past the frame; no rows: nothing to do, nothing read
    assert L.rtsResolveAsync(h, offs, idp, 2, 1, H, rgba.data_ptr(), None) == -1
    assert "outside the frame" in _native.last_error()
    assert L.rtsResolveAsync(h, offs, idp, 2, H + 1, 0, rgba.data_ptr(), None) == -1
    assert "outside the frame" in _native.last_error()
    assert L.rtsResolveAsync(h, None, None, 2, 0, 0, None, None) == 0
    assert L.rtsResolveAsync(h, None, None, 2, H, 0, None, None) == 0
    with pytest.raises(SrtError, match="outside the frame"):
        rig.scene.resolve([o[:10] for o in off], [i[:10] for i in ids], rgba[:10], row_begin=H - 5, row_count=10)
    # the wrapper's checks: the number of planes, list lengths, shape, dtype, device, contiguity
    with pytest.raises(ValueError):
        rig.scene.resolve([], [], rgba)
    with pytest.raises(ValueError):
        rig.scene.resolve(off * 9, ids * 9, rgba)
    with pytest.raises(ValueError):
        rig.scene.resolve(off, ids[:1], rgba)
    with pytest.raises(ValueError):
        rig.scene.render_samples(off[:1], ids, rgba)
    with pytest.raises(ValueError):
        rig.scene.resolve([off[0], off[1][:, :-1]], ids, rgba)
    with pytest.raises(ValueError):
        rig.scene.resolve(off, [ids[0], ids[1].to(torch.int64)], rgba)
    with pytest.raises(ValueError):
        rig.scene.resolve(off, ids, torch.zeros((H, W, 3), **f32))
    with pytest.raises(ValueError):
        rig.scene.resolve(off, ids, rgba.to(torch.float64))
    with pytest.raises(ValueError):
        rig.scene.resolve([off[0].cpu(), off[1]], ids, rgba)
    with pytest.raises(ValueError):
        rig.scene.render_samples(off, ids, rgba.cpu())
    with pytest.raises(ValueError):
        rig.scene.resolve(off, [ids[0], torch.zeros((W, H), dtype=torch.int32, device="cuda").t()], rgba)
    with pytest.raises(ValueError):
        rig.scene.render_samples(off, ids, torch.zeros((H, W, 8), **f32)[..., ::2])
    with pytest.raises(KeyError):
        rig.scene.render_samples(off, ids, rgba, variant="nope")
    # a valid call still works afterwards
    s_off, s_ids, _, resolved = frame_s
    got = rig.resolve(s_off, s_ids)
    rig.close()
    sc.same_bits("a valid call after the errors", got, resolved)
