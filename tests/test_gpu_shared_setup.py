"""The shared cull setup (render.h CullSetup; env SRT_SETUP): records, bins and work plan of a
whole-frame binned trace built once per prepared frame, every later frame running its tile
classification and the trace against that one read-only copy.

Every comparison is bit for bit on the uint32 view against the `lds` brute-force variant of the same
library (one fresh scene per reference), some also against the CPU oracle under assert_parity. The
setup counters -- builds of the shared setup, frames traced on it, frames traced with a per-frame
setup, which the library prints to stderr under SRT_SETUP_LOG=1 -- keep the tests from passing on the
per-frame path.

Shapes: soup2k at 200 x 150 -- 4 x 10 tiles of 64 x 16 with a partial last tile column and a partial
last tile row -- and at 333 x 170 for re-prepares.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

from scenefile import write_custom_scene
from test_gpu_parity import assert_parity, oracle_render

pytestmark = pytest.mark.gpu

W, H = 200, 150
W2, H2 = 333, 170


def make_inputs(w, h, seed=41):
    """Named sample-offset frames: in range (the shared lists hold), out of range for every tile, and
    out of range for one tile only (that tile alone streams every record)."""
    rng = np.random.default_rng(seed)
    rnd = rng.random((h, w, 2), dtype=np.float32)
    nan = rng.random((h, w, 2), dtype=np.float32)
    nan[20:28, 70:90] = np.nan  # inside tile (column 1, row 1)
    above = rng.random((h, w, 2), dtype=np.float32)
    above[50, 130, 0] = np.nextafter(np.float32(1), np.float32(2))  # one pixel just past the analytic box
    ends = rng.integers(0, 2, (h, w, 2)).astype(np.float32)  # exactly 0.0 and 1.0: the box's inclusive ends
    return {"half": np.full((h, w, 2), 0.5, np.float32), "rnd": rnd, "far": np.full((h, w, 2), -3.25, np.float32),
            "nan": nan, "above": above, "ends": ends}


class Rig:
    """One scene on cuda:0 and its stream; trace() returns the band as a numpy array."""

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

    def trace(self, offsets, variant="cull", r0=0, rows=None):
        torch = self.torch
        rows = self.h - r0 if rows is None else rows
        off = torch.from_numpy(np.ascontiguousarray(offsets[r0:r0 + rows])).cuda()
        out = torch.full((rows, self.w, 4), float("nan"), dtype=torch.float32, device="cuda")
        self.scene.trace(off, out, r0, rows, variant=variant, stream=self.stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def stats(self, capfd):
        """The scene's counters as its last binned cull call logged them (SRT_SETUP_LOG=1): everything
        captured on stderr since the previous look is this rig's, the references trace `lds` only."""
        lines = re.findall(r"srt setup: scene \S+ builds (\d+) shared_frames (\d+) per_frame_frames (\d+)",
                           capfd.readouterr().err)
        assert lines, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
        return tuple(int(v) for v in lines[-1])

    def close(self):
        self.scene.close()


def lds_refs(path, w, h, inputs):
    """The brute-force frame of every input, from a scene of its own."""
    rig = Rig(path, w, h)
    refs = {k: rig.trace(v, variant="lds") for k, v in inputs.items()}
    rig.close()
    return refs


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def soup_refs(scenes):
    inputs = make_inputs(W, H)
    return inputs, lds_refs(scenes["soup2k"], W, H, inputs)


SEQUENCE = ("half", "rnd", "far", "nan", "above", "ends", "half")


def test_alternating_offsets_one_setup(gpu, scenes, soup_refs, monkeypatch, capfd):
    """One scene, prepared once: in-range, out-of-range and partly out-of-range frames in turn, twice
    around, all on ONE build of the setup and none on a per-frame one."""
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    monkeypatch.delenv("SRT_SETUP", raising=False)
    inputs, refs = soup_refs
    oracle = {k: oracle_render(scenes["soup2k"], W, H, inputs[k]) for k in ("half", "rnd")}
    rig = Rig(scenes["soup2k"], W, H)
    for rep in range(2):
        for k in SEQUENCE:
            got = rig.trace(inputs[k])
            assert same(got, refs[k]), (rep, k)
            if rep == 0 and k in oracle:
                assert_parity(got, oracle[k])
    assert rig.stats(capfd) == (1, 2 * len(SEQUENCE), 0)
    rig.close()


def test_batches_equal_single_frames(gpu, scenes, soup_refs, monkeypatch, capfd):
    """trace_batch of 3 frames (parameters as kernel arguments) and engine launches of 9 (more than
    kMaxBatch: the device table), mixing the inputs: each frame equals its single-frame trace."""
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    import torch

    from simpleraytracer_amd.engine import FrameEngine

    monkeypatch.delenv("SRT_SETUP", raising=False)
    inputs, refs = soup_refs
    rig = Rig(scenes["soup2k"], W, H)
    single = {k: rig.trace(inputs[k]) for k in inputs}
    for k in inputs:
        assert same(single[k], refs[k]), k
    names = ("rnd", "nan", "half")
    off = [torch.from_numpy(inputs[k]).cuda() for k in names]
    out = [torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in names]
    rig.scene.trace_batch(off, out, 0, H, variant="cull", stream=rig.stream)
    torch.cuda.synchronize()
    for k, o in zip(names, out):
        assert same(o.cpu().numpy(), single[k]), k
    builds, shared, per_frame = rig.stats(capfd)
    # (a launch of 3 frames may get another trace grid than one frame's: a second build, never more)
    assert (shared, per_frame) == (len(inputs) + 3, 0) and 1 <= builds <= 2
    rig.close()
    nine = ("half", "rnd", "far", "nan", "above", "ends", "rnd", "half", "nan")
    with FrameEngine(scenes["soup2k"], W, H, devices=[0], batch=9, launch=9, queues=2) as e:
        e.set_inputs(np.stack([inputs[k] for k in nine]))
        e.run(2)
        for f in range(18):
            assert same(e.read_frame(f), single[nine[f % 9]]), f


@pytest.mark.parametrize("env", [{"SRT_CULL_CHUNK": "64"}, {"SRT_CULL_BIN_CAP": "8"},
                                 {"SRT_CULL_CHUNK": "64", "SRT_CULL_BIN_CAP": "8"}, {"SRT_CULL_CHUNKS": "16"}])
def test_chunking_and_overflow(gpu, scenes, soup_refs, monkeypatch, env, capfd):
    """Split parts (small chunks, a forced trace grid) and overflowed lists (capacity 8: those tiles'
    descriptors say FULL and stream every record) from the shared plan, in range and out of range."""
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    monkeypatch.delenv("SRT_SETUP", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    inputs, refs = soup_refs
    rig = Rig(scenes["soup2k"], W, H)
    for k in ("rnd", "far", "nan", "rnd"):
        assert same(rig.trace(inputs[k]), refs[k]), k
    assert rig.stats(capfd) == (1, 4, 0)
    rig.close()


def test_nasty_geometry(gpu, tmp_path, monkeypatch, capfd):
    """Behind the eye, degenerate and zero-area triangles, empty sky tiles (the baked empty flag and
    its FULL override), and frame-covering triangles: two of them (a large list of at most 4: the
    empty test runs) and six (more than 4: it does not)."""
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    monkeypatch.delenv("SRT_SETUP", raising=False)
    rng = np.random.default_rng(3)
    w, h = 200, 150
    small = []
    for _ in range(150):  # small triangles in the lower left of the view: the rest is sky
        c = rng.uniform([-0.9, -0.7, 3.0], [-0.2, -0.1, 5.0])
        small.append(list((c + rng.uniform(-0.08, 0.08, (3, 3))).ravel()))
    for _ in range(40):  # behind the eye
        small.append(list(rng.uniform([-1, -1, -6], [1, 1, -0.5], (3, 3)).ravel()))
    p = [0.3, 0.2, 4.0]
    small.append(p + p + p)  # a point
    small.append([0.0, 0.0, 4.0, 0.2, 0.2, 4.0, 0.4, 0.4, 4.0])  # collinear: zero area
    small.append([0.1, 0.1, 3.0, 0.1, 0.1, 3.0, 0.5, 0.2, 3.0])  # two equal vertices
    # far away, wider than the view's left half: binned to every tile it spans (the large list)
    cover = [[-30.0, -20.0, 9.0 + i, -0.05 * i, -20.0, 9.0 + i, -30.0, 40.0, 9.0 + i] for i in range(6)]
    inputs = make_inputs(w, h, seed=5)
    for n_cover in (2, 6):
        tris = small + cover[:n_cover]
        albedo = rng.uniform(0.2, 1.0, (len(tris), 3))
        path = write_custom_scene(tmp_path / f"nasty{n_cover}.srt", tris, albedo)
        refs = lds_refs(path, w, h, {k: inputs[k] for k in ("half", "far", "rnd", "nan")})
        assert (refs["half"][..., 3] == -1).mean() > 0.2  # sky
        rig = Rig(path, w, h)
        for k in ("half", "far", "rnd", "nan", "half"):
            assert same(rig.trace(inputs[k]), refs[k]), (n_cover, k)
        assert rig.stats(capfd) == (1, 5, 0)
        rig.close()
        assert_parity(refs["rnd"], oracle_render(path, w, h, inputs["rnd"]))


def test_reprepare_and_mixed_paths(gpu, scenes, soup_refs, monkeypatch, capfd):
    """A new shape rebuilds the setup, never stale; bands run on the per-frame setup between whole
    frames; the lds and unbinned record passes (edge slot 0) leave the shared copy alone."""
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    monkeypatch.delenv("SRT_SETUP", raising=False)
    inputs, refs = soup_refs
    inputs2 = {k: v for k, v in make_inputs(W2, H2, seed=43).items() if k in ("rnd", "nan")}
    refs2 = lds_refs(scenes["soup2k"], W2, H2, inputs2)
    rig = Rig(scenes["soup2k"], W, H)
    assert same(rig.trace(inputs["rnd"]), refs["rnd"])
    rig.prepare(W2, H2)
    for k in inputs2:
        assert same(rig.trace(inputs2[k]), refs2[k]), k
    rig.prepare(W, H)
    assert same(rig.trace(inputs["nan"]), refs["nan"])
    assert rig.stats(capfd) == (3, 4, 0)
    rig.prepare(W, H)  # the same frame again: no rebuild
    assert same(rig.trace(inputs["rnd"]), refs["rnd"])
    assert same(rig.trace(inputs["rnd"], r0=40, rows=77), refs["rnd"][40:117])
    assert same(rig.trace(inputs["ends"]), refs["ends"])
    assert rig.stats(capfd) == (3, 6, 1)
    assert same(rig.trace(inputs["rnd"], variant="lds"), refs["rnd"])
    assert same(rig.trace(inputs["above"]), refs["above"])
    monkeypatch.setenv("SRT_CULL_BIN", "0")  # unbinned cull: the record pass into edge slot 0
    assert same(rig.trace(inputs["half"]), refs["half"])
    monkeypatch.delenv("SRT_CULL_BIN")
    assert same(rig.trace(inputs["half"]), refs["half"])
    assert rig.stats(capfd) == (3, 8, 1)
    rig.close()


def test_modes_agree(gpu, scenes, soup_refs, monkeypatch, capfd):
    """SRT_SETUP {prepare, frame} x SRT_TRACE_RECORDS {stored, recompute}: one frame; junk raises."""
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    import simpleraytracer_amd as srt

    inputs, refs = soup_refs
    for setup in ("prepare", "frame"):
        for records in ("stored", "recompute"):
            monkeypatch.setenv("SRT_SETUP", setup)
            monkeypatch.setenv("SRT_TRACE_RECORDS", records)
            rig = Rig(scenes["soup2k"], W, H)
            for k in ("rnd", "nan"):
                assert same(rig.trace(inputs[k]), refs[k]), (setup, records, k)
            assert rig.stats(capfd) == ((1, 2, 0) if setup == "prepare" else (0, 0, 2))
            rig.close()
    monkeypatch.setenv("SRT_SETUP", "junk")
    rig = Rig(scenes["soup2k"], W, H)
    with pytest.raises(srt.SrtError, match="SRT_SETUP"):
        rig.trace(inputs["half"])
    rig.close()


def test_engine_on_the_shared_setup(gpu, scenes, monkeypatch):
    """FrameEngine, two queues, batches of 4, three steps: verified against another variant, and
    frame for frame the SRT_SETUP=frame engine's output."""
    from simpleraytracer_amd.engine import FrameEngine

    inputs = np.random.default_rng(77).random((8, H, W, 2), dtype=np.float32)
    inputs[3, 20:28, 70:90] = np.nan
    inputs[5] = -3.25
    frames = {}
    for setup in ("prepare", "frame"):
        monkeypatch.setenv("SRT_SETUP", setup)
        with FrameEngine(scenes["soup2k"], W, H, devices=[0], batch=4, queues=2) as e:
            e.set_inputs(inputs)
            e.run(3)
            bad, checked = e.verify()
            assert bad == 0 and checked > 0
            frames[setup] = [e.read_frame(k) for k in range(4, 12)]
    for a, b in zip(frames["prepare"], frames["frame"]):
        assert same(a, b)
