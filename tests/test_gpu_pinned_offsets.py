"""Pinned offsets (include/srt_pins.h rtnPinOffsetsAsync; DeviceScene.pin_offsets): the tile facts
of a whole-frame sample-offset buffer computed once and kept by the scene, so that the whole-frame
traces given that buffer run no facts launch.

Shapes and inputs are tests/test_gpu_shared_setup.py's: soup2k at 200 x 150 (4 x 10 tiles of 64 x 16
with a partial last tile column and row), 333 x 170 for the re-prepare, and make_inputs' half, rnd,
far, nan, above and ends, which together reach every combination of the facts' flags. Every frame is
compared bit for bit on the uint32 view with the `lds` brute-force variant of a fresh scene. The
counters the library prints under SRT_SETUP_LOG=1 -- pinned_frames: frames whose trace read a pin's
facts; facts_launches: facts launches issued, one per PinOffsets and one per shared launch with an
unpinned frame -- keep a test from passing on the wrong path.

A pinned tensor is kept alive, and unpinned, by the test that pinned it: the scene keys a pin by the
address, and torch's allocator hands a freed address out again.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

from test_gpu_shared_setup import H2, W2, H, W, Rig, lds_refs, make_inputs, same

pytestmark = pytest.mark.gpu

NAMES = ("half", "rnd", "far", "nan", "above", "ends")
CAMERA_B = (0.8, 0.4, -0.5, 0.0, 0.0, 3.0, 0.1, 1.0, 0.0, 50.0)  # the soup (z in [2, 4]) seen from the side

LOG = re.compile(r"srt setup: scene (\S+) builds (\d+) shared_frames (\d+) per_frame_frames (\d+) .*"
                 r"pinned_frames (\d+) facts_launches (\d+)")


@pytest.fixture(scope="module")
def refs(scenes):
    inputs = make_inputs(W, H)
    return inputs, lds_refs(scenes["soup2k"], W, H, inputs)


@pytest.fixture(autouse=True)
def log_on(monkeypatch):
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    for k in ("SRT_SETUP", "SRT_FACTS_PINS", "SRT_EMPTY_FILL", "SRT_FACTS_KERNEL"):
        monkeypatch.delenv(k, raising=False)


def counters(capfd):
    """Per scene, (shared_frames, per_frame_frames, pinned_frames, facts_launches) of its last log line
    since the previous look; the `lds` references log nothing."""
    out = {}
    for scene, _builds, shared, per_frame, pinned, launches in LOG.findall(capfd.readouterr().err):
        out[scene] = (int(shared), int(per_frame), int(pinned), int(launches))
    assert out, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
    return out


def one(capfd):
    """The counters of the only scene that logged."""
    c = counters(capfd)
    assert len(c) == 1, c
    return next(iter(c.values()))


def device_inputs(inputs, names=NAMES):
    import torch

    return {k: torch.from_numpy(inputs[k]).cuda() for k in names}


def trace(rig, off, r0=0, rows=None, local=False):
    """rig.trace for an offsets tensor that stays where it is (a pin is keyed by its address).
    local: the band's offsets are the tensor's first rows -- the tensor's own address."""
    torch = rig.torch
    rows = rig.h - r0 if rows is None else rows
    band = off[:rows] if local else off[r0:r0 + rows]
    out = torch.full((rows, rig.w, 4), float("nan"), dtype=torch.float32, device="cuda")
    rig.scene.trace(band, out, r0, rows, variant="cull", stream=rig.stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def trace_batch(rig, offs):
    torch = rig.torch
    outs = [torch.full((rig.h, rig.w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in offs]
    rig.scene.trace_batch(list(offs), outs, 0, rig.h, variant="cull", stream=rig.stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def test_parity(gpu, scenes, refs, monkeypatch, capfd):
    """Every input traced pinned, traced with SRT_FACTS_PINS=0 and the lds reference: all equal. The
    pinned traces issue no facts launch, the others one each."""
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device_inputs(inputs)
    for k in NAMES:
        rig.scene.pin_offsets(dev[k], rig.stream)
    _, _, pinned0, launches0 = one(capfd)
    assert (pinned0, launches0) == (0, len(NAMES))  # the pins' own launches
    for k in NAMES:
        assert same(trace(rig, dev[k]), ref[k]), k
    shared, per_frame, pinned, launches = one(capfd)
    assert (shared, per_frame, pinned, launches) == (len(NAMES), 0, len(NAMES), launches0)
    monkeypatch.setenv("SRT_FACTS_PINS", "0")
    for i, k in enumerate(NAMES):
        assert same(trace(rig, dev[k]), ref[k]), k
        assert one(capfd)[2:] == (len(NAMES), launches0 + i + 1), k
    monkeypatch.delenv("SRT_FACTS_PINS")
    for k in NAMES:  # and pinned again, after the unpinned traces rewrote the slot's own facts
        assert same(trace(rig, dev[k]), ref[k]), k
    assert one(capfd)[2:] == (2 * len(NAMES), launches0 + len(NAMES))
    for k in NAMES:
        rig.scene.unpin_offsets(dev[k])
    rig.close()


def test_batches_of_three(gpu, scenes, refs, capfd):
    """trace_batch of 3: all pinned (no facts launch), one pinned in every position (one launch over
    the two others), and one pinned buffer used by two frames of the batch."""
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device_inputs(inputs)
    for k in ("rnd", "nan", "half"):
        rig.scene.pin_offsets(dev[k], rig.stream)
    assert one(capfd)[2:] == (0, 3)
    names = ("rnd", "nan", "half")
    for k, got in zip(names, trace_batch(rig, [dev[k] for k in names])):
        assert same(got, ref[k]), k
    assert one(capfd)[2:] == (3, 3)  # three pinned frames, no launch
    pinned, launches = 3, 3
    for pos in range(3):  # `nan` pinned at `pos`, two unpinned inputs around it
        names = ["far", "above"]
        names.insert(pos, "nan")
        for k, got in zip(names, trace_batch(rig, [dev[k] for k in names])):
            assert same(got, ref[k]), (pos, k)
        pinned, launches = pinned + 1, launches + 1
        assert one(capfd)[2:] == (pinned, launches), pos
    names = ("half", "ends", "half")  # one pin serving two frames of the launch
    for k, got in zip(names, trace_batch(rig, [dev[k] for k in names])):
        assert same(got, ref[k]), k
    assert one(capfd)[2:] == (pinned + 2, launches + 1)
    for k in ("rnd", "nan", "half"):
        rig.scene.unpin_offsets(dev[k])
    rig.close()


def test_engine_nine_frames_per_launch(gpu, scenes, refs, capfd):
    """Launches of 9 frames read their parameters from the device table: two pinned inputs on one
    device, every frame right, and no facts launch after set_inputs' pins."""
    from simpleraytracer_amd.engine import FrameEngine

    inputs, ref = refs
    two = ("nan", "rnd")
    with FrameEngine(scenes["soup2k"], W, H, devices=[0], batch=9, launch=9, queues=2) as e:
        e.set_inputs(np.stack([inputs[k] for k in two]))
        after_pins = counters(capfd)
        e.run(2)
        for f in range(18):
            assert same(e.read_frame(f), ref[two[f % 2]]), f
        after_run = counters(capfd)
        assert len(after_run) == 2  # one scene per queue, one launch of 9 frames each
        for scene, c in after_run.items():
            assert after_pins[scene][3] == 2, after_pins  # the two pins' own launches
            assert tuple(x - y for x, y in zip(c, after_pins[scene])) == (9, 0, 9, 0), (after_pins, after_run)


def test_new_contents(gpu, scenes, refs, capfd):
    """A pin again announces new contents; an unpin brings the facts launch back; the engine's second
    set_inputs, whose allocation may land at the first one's address, gives the second inputs' frames."""
    from simpleraytracer_amd.engine import FrameEngine

    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    buf = device_inputs(inputs, ("half",))["half"]
    rig.scene.pin_offsets(buf, rig.stream)
    assert same(trace(rig, buf), ref["half"])
    buf.copy_(rig.torch.from_numpy(inputs["far"]))  # the same tensor, other contents
    rig.scene.pin_offsets(buf, rig.stream)
    assert same(trace(rig, buf), ref["far"])
    assert one(capfd)[2:] == (2, 2)
    rig.scene.unpin_offsets(buf)
    assert same(trace(rig, buf), ref["far"])
    assert one(capfd)[2:] == (2, 3)  # not pinned: its own facts launch
    rig.scene.unpin_offsets(buf)  # not pinned: nothing
    rig.close()
    with FrameEngine(scenes["soup2k"], W, H, devices=[0], batch=2, queues=2) as e:
        e.set_inputs(inputs["half"])
        first = counters(capfd)
        e.run(2)
        for f in range(4):
            assert same(e.read_frame(f), ref["half"]), f
        e.set_inputs(inputs["nan"])
        e.run(2)
        for f in range(4, 8):  # (the engine's frame count runs on: the resident frames are the last two batches')
            assert same(e.read_frame(f), ref["nan"]), f
        last = counters(capfd)
        assert len(last) == 2  # one scene per queue
        for scene, c in last.items():  # 2 + 2 pinned frames, and the second set_inputs' pin
            assert tuple(x - y for x, y in zip(c, first[scene])) == (4, 0, 4, 1), (first, last)


def test_reprepare(gpu, scenes, refs, capfd):
    """Prepare at the same size under another camera keeps the pins (facts do not depend on the
    camera); at another size it drops them, the traces compute their facts, and pinning again works."""
    import simpleraytracer_amd as srt

    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device_inputs(inputs, ("rnd", "nan"))
    for k in dev:
        rig.scene.pin_offsets(dev[k], rig.stream)
    assert same(trace(rig, dev["nan"]), ref["nan"])
    moved = srt.DeviceScene(scenes["soup2k"], 0, camera=CAMERA_B)  # the references under the other camera
    moved.prepare(W, H, rig.stream)
    ref_b = {}
    for k in dev:
        out = rig.torch.empty((H, W, 4), dtype=rig.torch.float32, device="cuda")
        moved.trace(dev[k], out, 0, H, variant="lds", stream=rig.stream)
        rig.torch.cuda.synchronize()
        ref_b[k] = out.cpu().numpy()
    moved.close()
    assert (ref_b["rnd"][..., 3] >= 0).any() and not same(ref_b["rnd"], ref["rnd"])
    rig.scene.set_camera(CAMERA_B, stream=rig.stream)
    rig.prepare(W, H)
    for k in dev:
        assert same(trace(rig, dev[k]), ref_b[k]), k
    assert one(capfd)[2:] == (3, 2)  # every trace pinned; the two pins' launches only
    rig.close()

    inputs2 = {k: v for k, v in make_inputs(W2, H2, seed=43).items() if k in ("rnd", "nan")}
    refs2 = lds_refs(scenes["soup2k"], W2, H2, inputs2)
    rig = Rig(scenes["soup2k"], W, H)
    rig.scene.pin_offsets(dev["rnd"], rig.stream)
    assert same(trace(rig, dev["rnd"]), ref["rnd"])
    assert one(capfd)[2:] == (1, 1)
    rig.prepare(W2, H2)  # another tile grid: the pins are gone
    dev2 = device_inputs(inputs2, ("rnd", "nan"))
    for k in dev2:
        assert same(trace(rig, dev2[k]), refs2[k]), k
    assert one(capfd)[2:] == (1, 3)
    rig.scene.pin_offsets(dev2["nan"], rig.stream)
    assert same(trace(rig, dev2["nan"]), refs2["nan"])
    assert one(capfd)[2:] == (2, 4)
    rig.prepare(W, H)  # and back: the old size's pin did not survive either
    assert same(trace(rig, dev["rnd"]), ref["rnd"])
    assert one(capfd)[2:] == (2, 5)
    rig.close()


def test_paths_that_ignore_pins(gpu, scenes, refs, monkeypatch, capfd):
    """A band, SRT_SETUP=frame, SRT_EMPTY_FILL=facts and SRT_FACTS_KERNEL=lean|block given a pinned
    pointer compute their own facts: right frames, pinned_frames unchanged."""
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device_inputs(inputs, ("nan", "above", "half"))
    for k in dev:
        rig.scene.pin_offsets(dev[k], rig.stream)
    for k in ("nan", "above"):
        assert same(trace(rig, dev[k]), ref[k]), k
    assert one(capfd) == (2, 0, 2, 3)
    # The pinned address itself as a band's offsets (band-local rows; uniform, so any rows serve), and
    # bands whose offsets start inside the pinned tensors.
    assert same(trace(rig, dev["half"], r0=16, rows=32, local=True), ref["half"][16:48])
    for k in ("nan", "above"):
        assert same(trace(rig, dev[k], r0=16, rows=32), ref[k][16:48]), k
    assert one(capfd)[:3] == (2, 3, 2)
    monkeypatch.setenv("SRT_SETUP", "frame")
    for k in ("nan", "above"):
        assert same(trace(rig, dev[k]), ref[k]), k
    assert one(capfd)[:3] == (2, 5, 2)
    monkeypatch.delenv("SRT_SETUP")
    monkeypatch.setenv("SRT_EMPTY_FILL", "facts")
    for k in ("nan", "above"):
        assert same(trace(rig, dev[k]), ref[k]), k
    assert one(capfd) == (4, 5, 2, 5)  # on the shared setup, each with its own (filling) facts launch
    monkeypatch.delenv("SRT_EMPTY_FILL")
    for kernel in ("lean", "block"):  # a facts kernel asked for by name runs, pinned frames or not
        monkeypatch.setenv("SRT_FACTS_KERNEL", kernel)
        assert same(trace(rig, dev["above"]), ref["above"]), kernel
    assert one(capfd) == (6, 5, 2, 7)
    monkeypatch.delenv("SRT_FACTS_KERNEL")
    assert same(trace(rig, dev["nan"]), ref["nan"])
    assert one(capfd) == (7, 5, 3, 7)  # and the pin serves again
    for k in dev:
        rig.scene.unpin_offsets(dev[k])
    rig.close()


def test_errors(gpu, scenes, refs, monkeypatch):
    """An unprepared scene, a null pointer, one pin beyond the cap, and SRT_FACTS_PINS=junk."""
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.device import MAX_PINS

    inputs, ref = refs
    scene = srt.DeviceScene(scenes["soup2k"], 0)
    buf = torch.from_numpy(inputs["half"]).cuda()
    with pytest.raises(srt.SrtError, match="Prepare"):
        scene.pin_offsets(buf)
    scene.close()
    rig = Rig(scenes["soup2k"], W, H)
    with pytest.raises(srt.SrtError, match="Bad buffer argument"):
        rig.scene.pin_offsets(None)
    with pytest.raises(srt.SrtError, match="Bad buffer argument"):
        rig.scene.unpin_offsets(None)
    assert MAX_PINS >= 64
    many = torch.full((MAX_PINS + 1, H, W, 2), 0.5, dtype=torch.float32, device="cuda")
    for i in range(MAX_PINS):
        rig.scene.pin_offsets(many[i], rig.stream)
    with pytest.raises(srt.SrtError, match=f"at most {MAX_PINS} pinned"):
        rig.scene.pin_offsets(many[MAX_PINS], rig.stream)
    rig.scene.pin_offsets(many[3], rig.stream)  # a pinned pointer again is no new pin
    assert same(trace(rig, many[MAX_PINS - 1]), ref["half"])  # nothing was evicted, and the last pin is right
    rig.scene.unpin_offsets(many[0])
    rig.scene.pin_offsets(many[MAX_PINS], rig.stream)  # an unpin makes room
    monkeypatch.setenv("SRT_FACTS_PINS", "junk")
    with pytest.raises(srt.SrtError, match="SRT_FACTS_PINS"):
        trace(rig, many[1])
    monkeypatch.delenv("SRT_FACTS_PINS")
    assert same(trace(rig, many[1]), ref["half"])
    rig.close()  # (the scene goes with its pins before the tensor does)


def test_stage_timing_without_a_facts_launch(gpu, scenes, refs):
    """Stage timing over all-pinned launches: the bin stage is 0, the trace takes time, nothing raises."""
    from simpleraytracer_amd.engine import FrameEngine

    inputs, _ = refs
    with FrameEngine(scenes["soup2k"], W, H, devices=[0], batch=4, queues=2) as e:
        e.set_inputs(np.stack([inputs["rnd"], inputs["nan"]]))
        launches, _prep, bin_ms, kernel_ms = e.stage_times(launches=5, frames=4)
        assert launches == 5 and bin_ms == 0.0 and kernel_ms > 0.0
        e.run(1)
        bad, checked = e.verify()
        assert bad == 0 and checked > 0
