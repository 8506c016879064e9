"""The empty sweep of the shared setup (render.h CullSetup::sweep; env SRT_EMPTY_SWEEP, SRT_EMPTY_GROUP):
the plan lists its statically empty descriptors last, and the trace grid is one block per list
descriptor plus one sweep block per G empty ones, which stores their misses -- or traces, one after
another, those whose tile facts are not valid in the frame (offsets outside [0, 1], NaN), with the
plan's empty flag ignored.

Every comparison is bit for bit on the uint32 view against the `lds` brute-force variant of the same
library (a scene of its own per reference), the cornell frame also against the oracle's committed
golden ids. Every case runs with the sweep on and off and looks at the counters the library prints
under SRT_SETUP_LOG=1 (empty_descs, sweep_blocks), so that no case passes on a build that never swept,
or swept with the switch off.

Shapes: 200 x 72 -- 4 x 5 tiles of 64 x 16, a last tile column of 8 pixels and a last tile row of 8
rows -- with soup2k and a nasty-geometry scene that is sky outside its lower left, and 1100 x 40 --
18 x 3 tiles, a last column of 12 pixels, a last row of 8 rows -- whose sky fills more than two groups
of 16 descriptors.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from scenefile import write_custom_scene

pytestmark = pytest.mark.gpu

W, H = 200, 72
WW, WH = 1100, 40
W2, H2 = 333, 170
GOLDEN = Path(__file__).resolve().parent / "golden"
DEFAULT_GROUP = 16


def make_inputs(w, h, seed=41):
    """Named sample-offset frames: in range, out of range for every tile (every empty tile traced),
    and out of range or NaN for single tiles (traced beside filled ones of the same group): tile
    (0, 0), the partial last column's partial last row, one tile inside."""
    rng = np.random.default_rng(seed)
    rnd = rng.random((h, w, 2), dtype=np.float32)
    rnd2 = rng.random((h, w, 2), dtype=np.float32)
    nan = rng.random((h, w, 2), dtype=np.float32)
    nan[20:28, 70:90] = np.nan  # inside tile (column 1, row 1)
    nan[2, w - 70, 1] = np.nan  # a tile of the top row, right of the middle
    above = rng.random((h, w, 2), dtype=np.float32)
    above[h * 2 // 3, w * 2 // 3, 0] = np.nextafter(np.float32(1), np.float32(2))  # just past the analytic box
    below = rng.random((h, w, 2), dtype=np.float32)
    below[3, 3, 1] = -0.5  # tile (0, 0)
    below[h - 2, w - 5, 0] = 1.5  # the partial last column's partial last row
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

    def _up(self, offsets):
        return self.torch.from_numpy(np.ascontiguousarray(offsets)).cuda()

    def trace(self, offsets, variant="cull"):
        torch = self.torch
        out = torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda")
        self.scene.trace(self._up(offsets), out, 0, self.h, variant=variant, stream=self.stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def trace_ids(self, offsets):
        torch = self.torch
        out = torch.full((self.h, self.w), -7, dtype=torch.int32, device="cuda")
        self.scene.trace_ids(self._up(offsets), out, 0, self.h, stream=self.stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def trace_batch(self, offsets, ids=False):
        torch = self.torch
        off = [self._up(o) for o in offsets]
        if ids:
            out = [torch.full((self.h, self.w), -7, dtype=torch.int32, device="cuda") for _ in off]
        else:
            out = [torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in off]
        self.scene.trace_batch(off, out, 0, self.h, variant="cull", stream=self.stream, ids=ids)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]

    def close(self):
        self.scene.close()


STATS = re.compile(r"srt setup: scene (\S+) builds (\d+) shared_frames (\d+) per_frame_frames (\d+) "
                   r"stream_frames (\d+) stream_records (\d+) empty_descs (\d+) sweep_blocks (\d+)")
NAMES = ("builds", "shared", "per_frame", "stream", "records", "empty", "sweep")


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


def ids_of(frame):
    return frame[..., 3].astype(np.int32)


def set_sweep(monkeypatch, on, group=None):
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    monkeypatch.delenv("SRT_SETUP", raising=False)
    monkeypatch.setenv("SRT_EMPTY_SWEEP", "1" if on else "0")
    if group is None:
        monkeypatch.delenv("SRT_EMPTY_GROUP", raising=False)
    else:
        monkeypatch.setenv("SRT_EMPTY_GROUP", str(group))


def check_counters(s, on, frames, group=DEFAULT_GROUP, sky=False):
    """Every frame on the shared setup; the sweep's blocks are ceil(empty_descs / G), or none."""
    assert (s["shared"], s["per_frame"]) == (frames, 0), s
    if on:
        assert s["sweep"] == -(-s["empty"] // group), (s, group)
        assert not sky or s["sweep"] > 0, s
    else:
        assert s["sweep"] == 0, s
        assert not sky or s["empty"] > 0, s


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
    """Per case: path, frame size, inputs and their brute-force frames (computed once, never changed)."""
    nasty = nasty_scene(tmp_path_factory)
    out = {}
    for name, path, w, h in (("soup2k", scenes["soup2k"], W, H), ("nasty", nasty, W, H), ("wide", nasty, WW, WH)):
        inputs = make_inputs(w, h)
        out[name] = (path, w, h, inputs, lds_refs(path, w, h, inputs))
    assert (out["nasty"][4]["half"][..., 3] == -1).mean() > 0.2  # sky
    assert (out["wide"][4]["half"][..., 3] == -1).mean() > 0.5
    return out


SKY = {"soup2k": False, "nasty": True, "wide": True}


@pytest.mark.parametrize("group", [1, 3, 16, 64])
@pytest.mark.parametrize("name", ["soup2k", "nasty", "wide"])
def test_group_boundaries(gpu, rigs, monkeypatch, capfd, name, group):
    """One descriptor per sweep block, groups that do not divide the count, the default, and one
    partial group holding everything (200 x 72) or nearly (the wide frame). Sweep on and off give the
    brute-force frame; `below` has invalid sky tiles beside valid ones of the same group."""
    path, w, h, inputs, refs = rigs[name]
    frames = {}
    for on in (True, False):
        set_sweep(monkeypatch, on, group)
        rig = Rig(path, w, h)
        frames[on] = {k: rig.trace(inputs[k]) for k in ("rnd", "below", "half")}
        s = stats(capfd)
        assert s["builds"] == 1
        check_counters(s, on, 3, group, SKY[name])
        if name == "wide":  # a condition of the case: more empty descriptors than two default groups
            assert s["empty"] >= 2 * DEFAULT_GROUP + 1, s
        rig.close()
    for k in frames[True]:
        assert same(frames[True][k], refs[k]), k
        assert same(frames[False][k], frames[True][k]), k


SEQUENCE = ("half", "above", "nan", "rnd", "below", "far", "rnd2", "half")


@pytest.mark.parametrize("name", ["soup2k", "nasty", "wide"])
def test_validity_per_tile_and_per_frame(gpu, rigs, monkeypatch, capfd, name):
    """In-range frames alternate with frames that have single tiles outside [0, 1] or NaN (`below`,
    `nan`, `above`: traced by their sweep block beside the tiles it fills) and every tile outside
    (`far`: each sweep block traces its whole group): as single frames, and as one 8-frame launch
    with a different input per frame."""
    path, w, h, inputs, refs = rigs[name]
    for on in (True, False):
        set_sweep(monkeypatch, on)
        rig = Rig(path, w, h)
        for k in SEQUENCE:
            assert same(rig.trace(inputs[k]), refs[k]), (on, k)
        s = stats(capfd)
        assert s["builds"] == 1
        check_counters(s, on, len(SEQUENCE), sky=SKY[name])
        batch = rig.trace_batch([inputs[k] for k in SEQUENCE])
        for k, got in zip(SEQUENCE, batch):
            assert same(got, refs[k]), (on, "batch", k)
        s = stats(capfd)
        assert 1 <= s["builds"] <= 2  # (an 8-frame launch may get another trace grid: one rebuild)
        check_counters(s, on, 2 * len(SEQUENCE), sky=SKY[name])
        rig.close()


@pytest.mark.parametrize("name", ["nasty", "wide"])
def test_output_forms(gpu, rigs, monkeypatch, capfd, name):
    """The same frames as hit ids (single frames and an 8-frame launch) and, through an engine whose
    traces store packed ids that a deferred pass shades, as packed ids: each equal to the switch-off
    build's output of the same form and to the brute-force frame."""
    from simpleraytracer_amd.engine import FrameEngine

    path, w, h, inputs, refs = rigs[name]
    got = {}
    for on in (True, False):
        set_sweep(monkeypatch, on, 3)
        rig = Rig(path, w, h)
        single = [rig.trace_ids(inputs[k]) for k in SEQUENCE]
        batch = rig.trace_batch([inputs[k] for k in SEQUENCE], ids=True)
        check_counters(stats(capfd), on, 2 * len(SEQUENCE), 3, sky=True)
        rig.close()
        with FrameEngine(path, w, h, devices=[0], batch=8, launch=8, queues=2) as e:
            e.set_inputs(np.stack([inputs[k] for k in SEQUENCE]))
            e.run(2)
            packed = [e.read_frame(f) for f in range(16)]
        every = all_stats(capfd)
        assert all(s["per_frame"] == 0 and (s["sweep"] > 0) == on for s in every), every
        got[on] = (single, batch, packed)
    for i, k in enumerate(SEQUENCE):
        for form in (0, 1):
            assert np.array_equal(got[True][form][i], ids_of(refs[k])), (form, k)
            assert np.array_equal(got[True][form][i], got[False][form][i]), (form, k)
        for f in (i, i + 8):
            assert same(got[True][2][f], refs[k]), ("packed", f, k)
            assert same(got[True][2][f], got[False][2][f]), ("packed", f, k)


def test_launch_of_more_than_eight_frames(gpu, rigs, monkeypatch, capfd):
    """Engine launches of 9 frames: the trace reads its parameters, the two counts and the group
    among them, from the device table."""
    from simpleraytracer_amd.engine import FrameEngine

    path, w, h, inputs, refs = rigs["nasty"]
    nine = ("half", "rnd", "far", "nan", "above", "below", "rnd2", "half", "nan")
    for on in (True, False):
        set_sweep(monkeypatch, on)
        with FrameEngine(path, w, h, devices=[0], batch=9, launch=9, queues=2) as e:
            e.set_inputs(np.stack([inputs[k] for k in nine]))
            e.run(2)
            for f in range(18):
                assert same(e.read_frame(f), refs[nine[f % 9]]), (on, f)
        every = all_stats(capfd)
        assert sum(s["shared"] for s in every) >= 18 and all(s["per_frame"] == 0 for s in every), every
        for s in every:
            assert s["empty"] > 0 and s["sweep"] == (-(-s["empty"] // DEFAULT_GROUP) if on else 0), s


def test_two_grids_and_reprepare(gpu, rigs, monkeypatch, capfd):
    """A one-frame launch followed by an 8-frame launch (two trace grids, two builds), then another
    size and back: every build counts its own plan and every launch sweeps by those counts."""
    path, w, h, inputs, refs = rigs["nasty"]
    inputs2 = {k: v for k, v in make_inputs(W2, H2, seed=43).items() if k in ("rnd", "below")}
    refs2 = lds_refs(path, W2, H2, inputs2)
    for on in (True, False):
        set_sweep(monkeypatch, on, 3)
        rig = Rig(path, w, h)
        assert same(rig.trace(inputs["rnd"]), refs["rnd"])
        a = stats(capfd)
        check_counters(a, on, 1, 3, sky=True)
        names = ("rnd2", "nan", "half", "above", "rnd", "below", "far", "rnd2")
        for k, got in zip(names, rig.trace_batch([inputs[k] for k in names])):
            assert same(got, refs[k]), (on, "batch", k)
        b = stats(capfd)
        check_counters(b, on, 9, 3, sky=True)
        rig.prepare(W2, H2)
        for k in inputs2:
            assert same(rig.trace(inputs2[k]), refs2[k]), (on, k)
        c = stats(capfd)
        check_counters(c, on, 11, 3)  # (at this size the large list is too long for the empty test: nothing to sweep)
        assert c["builds"] == b["builds"] + 1 and c["empty"] != a["empty"]
        rig.prepare(w, h)
        assert same(rig.trace(inputs["below"]), refs["below"])
        d = stats(capfd)
        check_counters(d, on, 12, 3, sky=True)
        assert d["builds"] == c["builds"] + 1 and d["empty"] == a["empty"]
        rig.close()


@pytest.mark.parametrize("var,value", [("SRT_TRACE_STREAM", "0"), ("SRT_TRACE_RECORDS", "recompute"),
                                       ("SRT_CULL_BIN_CAP", "8")])
@pytest.mark.parametrize("name", ["soup2k", "nasty"])
def test_other_setups(gpu, rigs, monkeypatch, capfd, name, var, value):
    """Stream off, recomputed records and a forced list overflow (its tiles FULL in the plan), each
    with the sweep on: the counts are read and the grid is right without a stream."""
    path, w, h, inputs, refs = rigs[name]
    monkeypatch.setenv(var, value)
    for on in (True, False):
        set_sweep(monkeypatch, on)
        rig = Rig(path, w, h)
        for k in ("rnd", "nan", "far", "below", "rnd"):
            assert same(rig.trace(inputs[k]), refs[k]), (on, k)
        s = stats(capfd)
        assert s["builds"] == 1
        check_counters(s, on, 5, sky=SKY[name])
        if var != "SRT_CULL_BIN_CAP":
            assert (s["stream"], s["records"]) == (0, 0), s
        rig.close()


def test_cornell_has_nothing_to_sweep(gpu, scenes, monkeypatch, capfd):
    """Cornell at 192 x 108: the walls reach every tile, so no descriptor is empty and no sweep block
    is launched. Brute force, and the oracle's committed ids."""
    w, h = 192, 108
    golden = np.load(GOLDEN / "frames.npz")["c2_cornell_192x108__rgba"]
    inputs = {"half": np.full((h, w, 2), 0.5, np.float32),
              "rnd": np.random.default_rng(9).random((h, w, 2), dtype=np.float32)}
    refs = lds_refs(scenes["cornell"], w, h, inputs)
    assert np.array_equal(refs["half"][..., 3].view(np.uint32), golden[..., 3].view(np.uint32))
    for on in (True, False):
        set_sweep(monkeypatch, on)
        rig = Rig(scenes["cornell"], w, h)
        for k in ("half", "rnd", "half"):
            assert same(rig.trace(inputs[k]), refs[k]), (on, k)
        s = stats(capfd)
        check_counters(s, on, 3)
        assert (s["empty"], s["sweep"]) == (0, 0), s
        rig.close()


def test_junk_switches(gpu, rigs, monkeypatch):
    import simpleraytracer_amd as srt

    path, w, h, inputs, refs = rigs["nasty"]
    rig = Rig(path, w, h)
    for var, junk in (("SRT_EMPTY_SWEEP", "yes"), ("SRT_EMPTY_SWEEP", "2"), ("SRT_EMPTY_GROUP", "0"),
                      ("SRT_EMPTY_GROUP", "65"), ("SRT_EMPTY_GROUP", "many"), ("SRT_EMPTY_GROUP", "-4")):
        monkeypatch.setenv(var, junk)
        with pytest.raises(srt.SrtError, match=var):
            rig.trace(inputs["half"])
        monkeypatch.delenv(var)
    assert same(rig.trace(inputs["half"]), refs["half"])
    rig.close()
