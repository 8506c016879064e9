"""The shared setup's record stream (render.h kStreamCapRecords; env SRT_TRACE_STREAM): every
(tile, chunk) of the plan has its candidates' 64-B cull records contiguously, in the order the trace
walks them, and TraceCullKernel<.., STREAM> reads them from there -- the first batch requested beside
the frame's tile facts, before it is known whether the tile is in range.

Every comparison is bit for bit on the uint32 view against the `lds` brute-force variant of the same
library (a scene of its own per reference), the cornell frame also against the oracle's committed
golden ids. Every case runs with the stream on and off and looks at the counters the library prints
under SRT_SETUP_LOG=1 (stream_frames, stream_records), so that no case passes on a build that fell
back to the indexed path silently, or never streamed.

Shapes: soup2k and a nasty-geometry scene at 200 x 72 -- 4 x 5 tiles of 64 x 16, a last tile column
of 8 pixels and a last tile row of 8 rows --, 333 x 170 for re-prepares, cornell at 192 x 108 (its
walls are binned to every tile: large-list-only tiles). Frames that small leave the chip partly
idle, so the plan splits the parts into chunks by default; SRT_CULL_CHUNKS / SRT_CULL_CHUNK move the
chunk size across the 128-record batch.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from scenefile import write_custom_scene

pytestmark = pytest.mark.gpu

W, H = 200, 72
W2, H2 = 333, 170
GOLDEN = Path(__file__).resolve().parent / "golden"


def make_inputs(w, h, seed=41):
    """Named sample-offset frames: in range (the stream's ranges hold), out of range for every tile,
    and out of range or NaN for one tile only (that tile alone drops its first batch and streams
    every record)."""
    rng = np.random.default_rng(seed)
    rnd = rng.random((h, w, 2), dtype=np.float32)
    rnd2 = rng.random((h, w, 2), dtype=np.float32)
    nan = rng.random((h, w, 2), dtype=np.float32)
    nan[20:28, 70:90] = np.nan  # inside tile (column 1, row 1)
    above = rng.random((h, w, 2), dtype=np.float32)
    above[50, 130, 0] = np.nextafter(np.float32(1), np.float32(2))  # one pixel just past the analytic box
    below = rng.random((h, w, 2), dtype=np.float32)
    below[3, 3, 1] = -0.5  # tile (0, 0)
    below[70, 195, 0] = 1.5  # the partial last column's partial last row
    return {"half": np.full((h, w, 2), 0.5, np.float32), "rnd": rnd, "rnd2": rnd2,
            "far": np.full((h, w, 2), -3.25, np.float32), "nan": nan, "above": above, "below": below}


class Rig:
    """One scene on cuda:0 and its stream; trace() returns the frame as a numpy array."""

    def __init__(self, path, w, h):
        import torch

        import simpleraytracer_amd as srt

        self.torch = torch
        self.scene = srt.DeviceScene(path, 0)
        self.stream = torch.cuda.current_stream()
        self.prepare(w, h)

    def prepare(self, w, h):
        self.w, self.h = w, h
        self.scene.prepare(w, h, self.stream)

    def trace(self, offsets, variant="cull"):
        torch = self.torch
        off = torch.from_numpy(np.ascontiguousarray(offsets)).cuda()
        out = torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda")
        self.scene.trace(off, out, 0, self.h, variant=variant, stream=self.stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def trace_batch(self, offsets):
        torch = self.torch
        off = [torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in offsets]
        out = [torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in off]
        self.scene.trace_batch(off, out, 0, self.h, variant="cull", stream=self.stream)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]

    def close(self):
        self.scene.close()


STATS = re.compile(r"srt setup: scene (\S+) builds (\d+) shared_frames (\d+) per_frame_frames (\d+) "
                   r"stream_frames (\d+) stream_records (\d+)")
NAMES = ("builds", "shared", "per_frame", "stream", "records")


def all_stats(capfd):
    """The last counters of every scene that logged since the previous look."""
    last = {}
    for m in STATS.finditer(capfd.readouterr().err):
        last[m.group(1)] = dict(zip(NAMES, (int(v) for v in m.groups()[1:])))
    assert last, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
    return list(last.values())


def stats(capfd):
    """One scene's (the references trace `lds` only and log nothing)."""
    every = all_stats(capfd)
    assert len(every) == 1
    return every[0]


def lds_refs(path, w, h, inputs):
    rig = Rig(path, w, h)
    refs = {k: rig.trace(v, variant="lds") for k, v in inputs.items()}
    rig.close()
    return refs


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def set_stream(monkeypatch, on):
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    monkeypatch.delenv("SRT_SETUP", raising=False)
    monkeypatch.setenv("SRT_TRACE_STREAM", "1" if on else "0")


def check_counters(s, on, frames):
    """Every frame on the shared setup; all of them streamed from a stream that exists, or none."""
    assert (s["shared"], s["per_frame"]) == (frames, 0), s
    if on:
        assert s["stream"] == frames and s["records"] > 0 and s["records"] % 2 == 0, s
    else:
        assert (s["stream"], s["records"]) == (0, 0), s


def nasty_scene(tmp_path_factory):
    """Small triangles in the lower left (the rest is sky: statically empty tiles), triangles behind
    the eye, degenerate ones, and two far triangles wider than half the view (the large list; at most
    4 entries, so the empty test runs)."""
    rng = np.random.default_rng(3)
    tris = []
    for _ in range(150):
        c = rng.uniform([-0.9, -0.7, 3.0], [-0.2, -0.1, 5.0])
        tris.append(list((c + rng.uniform(-0.08, 0.08, (3, 3))).ravel()))
    for _ in range(40):
        tris.append(list(rng.uniform([-1, -1, -6], [1, 1, -0.5], (3, 3)).ravel()))
    p = [0.3, 0.2, 4.0]
    tris.append(p + p + p)
    tris.append([0.0, 0.0, 4.0, 0.2, 0.2, 4.0, 0.4, 0.4, 4.0])
    tris.append([0.1, 0.1, 3.0, 0.1, 0.1, 3.0, 0.5, 0.2, 3.0])
    tris += [[-30.0, -20.0, 9.0 + i, -0.05 * i, -20.0, 9.0 + i, -30.0, 40.0, 9.0 + i] for i in range(2)]
    albedo = rng.uniform(0.2, 1.0, (len(tris), 3))
    return write_custom_scene(tmp_path_factory.mktemp("nasty") / "nasty.srt", tris, albedo)


@pytest.fixture(scope="module")
def rigs(scenes, tmp_path_factory):
    """Per scene: path, inputs and their brute-force frames at W x H (computed once, never changed)."""
    inputs = make_inputs(W, H)
    out = {}
    for name, path in (("soup2k", scenes["soup2k"]), ("nasty", nasty_scene(tmp_path_factory))):
        out[name] = (path, inputs, lds_refs(path, W, H, inputs))
    assert (out["nasty"][2]["half"][..., 3] == -1).mean() > 0.2  # sky
    return out


@pytest.mark.parametrize("chunks", [2, 4, 16])
@pytest.mark.parametrize("name", ["soup2k", "nasty"])
def test_chunk_boundaries(gpu, rigs, monkeypatch, capfd, name, chunks):
    """Room for 2, 4 and 16 descriptors per part with a smallest chunk of 64: the plan's chunk is the
    power of two >= candidates / spare descriptors, so the three cut the parts into ranges of more
    than one 128-record batch, of about one batch, and of at most 64 records. Stream on and off give
    the brute-force frame."""
    monkeypatch.setenv("SRT_CULL_CHUNKS", str(chunks))
    monkeypatch.setenv("SRT_CULL_CHUNK", "64")
    path, inputs, refs = rigs[name]
    frames = {}
    for on in (True, False):
        set_stream(monkeypatch, on)
        rig = Rig(path, W, H)
        frames[on] = {k: rig.trace(inputs[k]) for k in ("rnd", "half", "rnd")}
        s = stats(capfd)
        assert s["builds"] == 1
        check_counters(s, on, 3)
        rig.close()
    for k in frames[True]:
        assert same(frames[True][k], refs[k]), k
        assert same(frames[False][k], frames[True][k]), k


SEQUENCE = ("half", "above", "nan", "rnd", "below", "far", "rnd2", "half")


@pytest.mark.parametrize("name", ["soup2k", "nasty"])
def test_mixed_ranges_on_one_prepared_scene(gpu, rigs, monkeypatch, capfd, name):
    """In-range frames alternate with frames that have a tile outside [0, 1], a tile with NaN offsets
    and every tile outside: as single frames, and as one 8-frame launch with a different input per
    frame. The first batch is dropped per tile and per frame, and the plan's empty flag ignored where
    a tile is out of range (nasty: the sky tiles of `far` and `below`)."""
    path, inputs, refs = rigs[name]
    for on in (True, False):
        set_stream(monkeypatch, on)
        rig = Rig(path, W, H)
        for k in SEQUENCE:
            assert same(rig.trace(inputs[k]), refs[k]), (on, k)
        s = stats(capfd)
        assert s["builds"] == 1
        check_counters(s, on, len(SEQUENCE))
        batch = rig.trace_batch([inputs[k] for k in SEQUENCE])
        for k, got in zip(SEQUENCE, batch):
            assert same(got, refs[k]), (on, "batch", k)
        s = stats(capfd)
        assert 1 <= s["builds"] <= 2  # (an 8-frame launch may get another trace grid: one rebuild)
        check_counters(s, on, 2 * len(SEQUENCE))
        rig.close()


def test_forced_list_overflow(gpu, rigs, monkeypatch, capfd):
    """Capacity 8: the overflowed tiles' descriptors say FULL, get no stream range (the stream is
    shorter than the unforced one) and stream every record."""
    path, inputs, refs = rigs["soup2k"]
    set_stream(monkeypatch, True)
    rig = Rig(path, W, H)
    assert same(rig.trace(inputs["rnd"]), refs["rnd"])
    unforced = stats(capfd)["records"]
    rig.close()
    monkeypatch.setenv("SRT_CULL_BIN_CAP", "8")
    for on in (True, False):
        set_stream(monkeypatch, on)
        rig = Rig(path, W, H)
        for k in ("rnd", "nan", "far", "rnd"):
            assert same(rig.trace(inputs[k]), refs[k]), (on, k)
        s = stats(capfd)
        assert (s["builds"], s["shared"], s["per_frame"]) == (1, 4, 0), s
        assert s["stream"] == (4 if on else 0) and s["records"] < unforced and s["records"] % 2 == 0, s
        rig.close()


def test_forced_cap_fallback(gpu, rigs, monkeypatch, capfd):
    """A stream longer than the cap is not built: the setup's frames run the indexed path and equal
    the streamed ones. The cap is part of the setup's key: lifting it rebuilds, with a stream."""
    import simpleraytracer_amd as srt

    path, inputs, refs = rigs["soup2k"]
    set_stream(monkeypatch, True)
    monkeypatch.setenv("SRT_TRACE_STREAM_CAP", "16")
    rig = Rig(path, W, H)
    capped = {k: rig.trace(inputs[k]) for k in ("rnd", "above")}
    s = stats(capfd)
    assert (s["builds"], s["shared"], s["per_frame"], s["stream"], s["records"]) == (1, 2, 0, 0, 0), s
    monkeypatch.delenv("SRT_TRACE_STREAM_CAP")
    for k in capped:
        got = rig.trace(inputs[k])
        assert same(got, capped[k]) and same(got, refs[k]), k
    s = stats(capfd)
    assert (s["builds"], s["shared"], s["stream"]) == (2, 4, 2) and s["records"] > 16, s
    for var, junk in (("SRT_TRACE_STREAM", "yes"), ("SRT_TRACE_STREAM", "2"), ("SRT_TRACE_STREAM_CAP", "lots")):
        monkeypatch.setenv(var, junk)
        with pytest.raises(srt.SrtError, match=var):
            rig.trace(inputs["half"])
        monkeypatch.delenv(var)
    rig.close()


def test_reprepare_never_reads_a_stale_stream(gpu, rigs, scenes, monkeypatch, capfd):
    """Size A, size B (another tile count), A again, then a one-frame launch followed by an 8-frame
    launch (another trace grid): every change rebuilds plan and stream."""
    path, inputs, refs = rigs["soup2k"]
    inputs2 = {k: v for k, v in make_inputs(W2, H2, seed=43).items() if k in ("rnd", "nan")}
    refs2 = lds_refs(path, W2, H2, inputs2)
    for on in (True, False):
        set_stream(monkeypatch, on)
        rig = Rig(path, W, H)
        assert same(rig.trace(inputs["rnd"]), refs["rnd"])
        a = stats(capfd)
        check_counters(a, on, 1)
        rig.prepare(W2, H2)
        for k in inputs2:
            assert same(rig.trace(inputs2[k]), refs2[k]), (on, k)
        b = stats(capfd)
        check_counters(b, on, 3)
        assert b["builds"] == 2 and (not on or b["records"] != a["records"])
        rig.prepare(W, H)
        assert same(rig.trace(inputs["nan"]), refs["nan"])
        assert same(rig.trace(inputs["rnd"]), refs["rnd"])
        s = stats(capfd)
        check_counters(s, on, 5)
        assert s["builds"] == 3 and s["records"] == a["records"]
        names = ("rnd2", "nan", "half", "above", "rnd", "below", "far", "rnd2")
        for k, got in zip(names, rig.trace_batch([inputs[k] for k in names])):
            assert same(got, refs[k]), (on, "batch", k)
        assert same(rig.trace(inputs["rnd"]), refs["rnd"])
        s = stats(capfd)
        check_counters(s, on, 14)
        assert s["builds"] in (3, 5)  # the 8-frame grid, and back: both rebuilt, or the grids are equal
        rig.close()


def test_launch_of_more_than_eight_frames(gpu, rigs, monkeypatch, capfd):
    """Engine launches of 9 frames: more than the kernel arguments hold, so the trace reads its
    parameters, the stream pointer among them, from the device table."""
    from simpleraytracer_amd.engine import FrameEngine

    path, inputs, refs = rigs["soup2k"]
    nine = ("half", "rnd", "far", "nan", "above", "below", "rnd2", "half", "nan")
    for on in (True, False):
        set_stream(monkeypatch, on)
        with FrameEngine(path, W, H, devices=[0], batch=9, launch=9, queues=2) as e:
            e.set_inputs(np.stack([inputs[k] for k in nine]))
            e.run(2)
            for f in range(18):
                assert same(e.read_frame(f), refs[nine[f % 9]]), (on, f)
        every = all_stats(capfd)
        assert sum(s["shared"] for s in every) >= 18 and all(s["per_frame"] == 0 for s in every), every
        for s in every:
            assert s["stream"] == (s["shared"] if on else 0) and (s["records"] > 0) == on, s


def test_queries_and_layers_between_streamed_traces(gpu, rigs, monkeypatch, capfd):
    """Point queries and depth layers read the setup's lists and records by position, between traces
    that read its stream: their answers are those of a stream-less scene, and the queries at the
    pixel centres are the frame's ids."""
    import torch

    path, inputs, refs = rigs["soup2k"]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    centres = np.stack([(xs + np.float32(0.5)) / np.float32(W), (ys + np.float32(0.5)) / np.float32(H)], -1)
    extra = np.array([[-0.25, 0.5], [0.5, 1.5], [np.nan, 0.2]], np.float32)  # streamed queries
    pos = torch.from_numpy(np.concatenate([centres.reshape(-1, 2), extra])).cuda()
    n = pos.shape[0]
    answers = {}
    for on in (False, True):
        set_stream(monkeypatch, on)
        rig = Rig(path, W, H)
        ids, t = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
        lid = torch.empty((3, n), dtype=torch.int32, device="cuda")
        lt = torch.empty((3, n), dtype=torch.float32, device="cuda")
        assert same(rig.trace(inputs["half"]), refs["half"])
        rig.scene.query(pos, ids, t, stream=rig.stream)
        assert same(rig.trace(inputs["nan"]), refs["nan"])
        rig.scene.layers(pos, lid, lt, stream=rig.stream)
        assert same(rig.trace(inputs["rnd"]), refs["rnd"])
        torch.cuda.synchronize()
        answers[on] = [a.cpu().numpy() for a in (ids, t, lid, lt)]
        s = stats(capfd)
        assert s["builds"] == 1  # queries, layers and one-frame traces share one build
        check_counters(s, on, 3)
        rig.close()
    for a, b in zip(answers[False], answers[True]):
        assert same(a, b)
    ids, _, lid, _ = answers[True]
    assert np.array_equal(ids[:H * W].reshape(H, W), refs["half"][..., 3].astype(np.int32))
    assert np.array_equal(lid[0], ids)


def test_cornell_large_list_tiles_and_golden_ids(gpu, scenes, monkeypatch, capfd):
    """Cornell at 192 x 108: the walls are binned to every tile, so tiles' ranges hold large-list
    records only or a bin list followed by them. Brute force, and the oracle's committed ids."""
    w, h = 192, 108
    golden = np.load(GOLDEN / "frames.npz")["c2_cornell_192x108__rgba"]
    inputs = {"half": np.full((h, w, 2), 0.5, np.float32),
              "rnd": np.random.default_rng(9).random((h, w, 2), dtype=np.float32)}
    refs = lds_refs(scenes["cornell"], w, h, inputs)
    assert np.array_equal(refs["half"][..., 3].view(np.uint32), golden[..., 3].view(np.uint32))
    for on in (True, False):
        set_stream(monkeypatch, on)
        rig = Rig(scenes["cornell"], w, h)
        for k in ("half", "rnd", "half"):
            assert same(rig.trace(inputs[k]), refs[k]), (on, k)
        check_counters(stats(capfd), on, 3)
        rig.close()
