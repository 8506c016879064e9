"""Regular launches (renderer.h PinOffsets): a shared launch whose frames are
all pinned, with a summary that says every tile is regular, usable and in range, runs the trace
kernel without the per-pixel position table. Every other launch runs the general kernel.

Shapes and inputs are tests/test_gpu_shared_setup.py's: soup2k at 200 x 150 (4 x 10 tiles of 64 x 16, a
last tile column 8 pixels wide, a last tile row 6 rows high), plus one 64 x 16 frame (a single tile)
and the same scene with SRT_CULL_CHUNK=64, which splits its heavy parts into chunks (the split the
blocking tests use). Every frame is compared bit for bit on the uint32 view with the `lds`
brute-force variant of a fresh scene, and with the same call under SRT_TRACE_POS=table. The counter
the library prints under SRT_SETUP_LOG=1 -- regular_launches: shared launches that took the regular
kernel -- is asserted in every case, so no test passes on the wrong path.

A summary is known once the work queued by pin_offsets has completed; a launch that finds it unknown
takes the general kernel (the same bits). The tests synchronise after pinning, so that which kernel a
launch takes is determined. A pinned tensor is kept alive, and unpinned, by the test that pinned it.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

from test_gpu_shared_setup import H, W, Rig, lds_refs, make_inputs, same

pytestmark = pytest.mark.gpu

LOG = re.compile(r"srt setup: scene (\S+) builds (\d+) shared_frames (\d+) per_frame_frames (\d+) .*"
                 r"pinned_frames (\d+) facts_launches (\d+) regular_launches (\d+)")

# The three shared forms of the trace, by the switches the shared-setup tests use.
FORMS = {"stream": {}, "indexed": {"SRT_TRACE_STREAM": "0"}, "recompute": {"SRT_TRACE_RECORDS": "recompute"}}


def tile_offsets(w, h, seed=7):
    """Regular per tile (64 x 16), with another in-range (ox, oy) in every tile."""
    rng = np.random.default_rng(seed)
    ty, tx = (h + 15) // 16, (w + 63) // 64
    per_tile = rng.random((ty, tx, 2), dtype=np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(per_tile, 16, axis=0), 64, axis=1)[:h, :w])


def regular_inputs(w, h):
    inputs = make_inputs(w, h)
    inputs["tiles"] = tile_offsets(w, h)
    ulp = np.full((h, w, 2), 0.5, np.float32)
    ulp[37, 101, 1] = np.nextafter(np.float32(0.5), np.float32(1))  # one pixel of tile (1, 2), one ulp off
    inputs["ulp"] = ulp
    return inputs


@pytest.fixture(scope="module")
def refs(scenes):
    inputs = regular_inputs(W, H)
    return inputs, lds_refs(scenes["soup2k"], W, H, inputs)


@pytest.fixture(autouse=True)
def log_on(monkeypatch):
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    for k in ("SRT_SETUP", "SRT_FACTS_PINS", "SRT_EMPTY_FILL", "SRT_FACTS_KERNEL", "SRT_TRACE_POS", "SRT_TRACE_STREAM",
              "SRT_TRACE_RECORDS", "SRT_CULL_CHUNK", "SRT_CULL_CHUNKS", "SRT_CULL_BIN_CAP"):
        monkeypatch.delenv(k, raising=False)


def counters(capfd):
    """Per scene, (shared_frames, pinned_frames, facts_launches, regular_launches) of its last log line."""
    out = {}
    for scene, _b, shared, _pf, pinned, launches, regular in LOG.findall(capfd.readouterr().err):
        out[scene] = (int(shared), int(pinned), int(launches), int(regular))
    assert out, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
    return out


def regular_count(capfd):
    c = counters(capfd)
    assert len(c) == 1, c
    return next(iter(c.values()))[3]


def pin(rig, tensor):
    rig.scene.pin_offsets(tensor, rig.stream)
    rig.torch.cuda.synchronize()  # the summary is known from here on (module docstring)


def launch(rig, offs):
    """One launch of len(offs) whole frames from tensors that stay where they are."""
    torch = rig.torch
    outs = [torch.full((rig.h, rig.w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in offs]
    if len(offs) == 1:
        rig.scene.trace(offs[0], outs[0], 0, rig.h, variant="cull", stream=rig.stream)
    else:
        rig.scene.trace_batch(list(offs), outs, 0, rig.h, variant="cull", stream=rig.stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def check(rig, dev, names, ref, monkeypatch, capfd, before, expect):
    """The launch of `names` gives the references' bits and counts `expect` regular launches; the same
    call under SRT_TRACE_POS=table gives the same bits and counts none. Returns the counter."""
    got = launch(rig, [dev[k] for k in names])
    after = regular_count(capfd)
    for k, g in zip(names, got):
        assert same(g, ref[k]), (names, k)
    assert after - before == expect, (names, before, after)
    monkeypatch.setenv("SRT_TRACE_POS", "table")
    table = launch(rig, [dev[k] for k in names])
    monkeypatch.delenv("SRT_TRACE_POS")
    assert regular_count(capfd) == after, names
    for k, g, t in zip(names, got, table):
        assert same(g, t), (names, k)
    return after


def device(rig, inputs, names):
    return {k: rig.torch.from_numpy(inputs[k]).cuda() for k in names}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_eligible(gpu, scenes, refs, monkeypatch, capfd, form):
    """Uniform and per-tile offsets, launches of 1 and 3 frames, in each form of the trace: regular."""
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device(rig, inputs, ("half", "tiles"))
    for t in dev.values():
        pin(rig, t)
    n = regular_count(capfd)
    assert n == 0
    for names in (("half",), ("tiles",), ("tiles", "half", "tiles")):
        n = check(rig, dev, names, ref, monkeypatch, capfd, n, 1)
    for t in dev.values():
        rig.scene.unpin_offsets(t)
    rig.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_engine_nine_frames(gpu, scenes, refs, monkeypatch, capfd, form):
    """Launches of 9 frames (more than kMaxBatch: the device table) of two eligible inputs: every launch
    regular, every frame right; under SRT_TRACE_POS=table none regular, the same frames."""
    from simpleraytracer_amd.engine import FrameEngine

    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    inputs, ref = refs
    two = ("tiles", "half")
    frames = {}
    for pos in ("auto", "table"):
        monkeypatch.setenv("SRT_TRACE_POS", pos)
        with FrameEngine(scenes["soup2k"], W, H, devices=[0], batch=9, launch=9, queues=2) as e:
            e.set_inputs(np.stack([inputs[k] for k in two]))
            after_pins = counters(capfd)
            e.run(2)
            frames[pos] = [e.read_frame(f) for f in range(18)]
            after_run = counters(capfd)
        assert len(after_run) == 2  # one scene per queue, one launch of 9 frames each
        for scene, c in after_run.items():
            shared, pinned, launches, regular = (x - y for x, y in zip(c, after_pins[scene]))
            assert (shared, pinned, launches) == (9, 9, 0), (after_pins, after_run)
            assert regular == (1 if pos == "auto" else 0), (pos, after_pins, after_run)
    for f in range(18):
        assert same(frames["auto"][f], ref[two[f % 2]]), f
        assert same(frames["auto"][f], frames["table"][f]), f


def test_single_tile(gpu, scenes, monkeypatch, capfd):
    """One 64 x 16 frame: a single tile, a grid of one list block or one sweep block."""
    w, h = 64, 16
    inputs = {"half": np.full((h, w, 2), 0.5, np.float32), "tiles": tile_offsets(w, h, seed=9)}
    ref = lds_refs(scenes["soup2k"], w, h, inputs)
    rig = Rig(scenes["soup2k"], w, h)
    dev = device(rig, inputs, ("half", "tiles"))
    for t in dev.values():
        pin(rig, t)
    n = regular_count(capfd)
    for names in (("half",), ("tiles",), ("half", "tiles", "half")):
        n = check(rig, dev, names, ref, monkeypatch, capfd, n, 1)
    rig.close()


@pytest.mark.parametrize("form", ["stream", "indexed"])
def test_split_chunks(gpu, scenes, refs, monkeypatch, capfd, form):
    """Parts split into chunks (the smallest chunk of 64, as the blocking tests force it): the split-chunk
    hand-off of the regular kernel, whose last chunk shades from the column and row tables."""
    monkeypatch.setenv("SRT_CULL_CHUNK", "64")
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device(rig, inputs, ("half", "tiles"))
    for t in dev.values():
        pin(rig, t)
    n = regular_count(capfd)
    for names in (("tiles",), ("half", "tiles", "tiles")):
        n = check(rig, dev, names, ref, monkeypatch, capfd, n, 1)
    rig.close()


@pytest.mark.parametrize("name", ["ulp", "rnd", "nan", "far", "above"])
def test_not_eligible_inputs(gpu, scenes, refs, monkeypatch, capfd, name):
    """One pixel one ulp off, random offsets, and the invalid inputs (regular or not): pinned, traced by
    the general kernel, alone and beside an eligible pin."""
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device(rig, inputs, (name, "half"))
    for t in dev.values():
        pin(rig, t)
    n = regular_count(capfd)
    n = check(rig, dev, (name,), ref, monkeypatch, capfd, n, 0)
    n = check(rig, dev, ("half", name, "half"), ref, monkeypatch, capfd, n, 0)  # an eligible pin with an ineligible one
    check(rig, dev, ("half",), ref, monkeypatch, capfd, n, 1)  # (and the eligible one alone is regular)
    rig.close()


def test_not_eligible_launches(gpu, scenes, refs, monkeypatch, capfd):
    """A pin beside an unpinned frame, SRT_TRACE_POS=table and SRT_FACTS_PINS=0: the general kernel."""
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device(rig, inputs, ("half", "tiles"))
    pin(rig, dev["half"])
    n = regular_count(capfd)
    n = check(rig, dev, ("half", "tiles"), ref, monkeypatch, capfd, n, 0)  # `tiles` is eligible, but not pinned
    n = check(rig, dev, ("tiles",), ref, monkeypatch, capfd, n, 0)
    pin(rig, dev["tiles"])
    n = regular_count(capfd)
    monkeypatch.setenv("SRT_FACTS_PINS", "0")
    n = check(rig, dev, ("half", "tiles"), ref, monkeypatch, capfd, n, 0)
    monkeypatch.delenv("SRT_FACTS_PINS")
    monkeypatch.setenv("SRT_TRACE_POS", "table")
    got = launch(rig, [dev["half"], dev["tiles"]])
    assert regular_count(capfd) == n
    assert same(got[0], ref["half"]) and same(got[1], ref["tiles"])
    monkeypatch.delenv("SRT_TRACE_POS")
    check(rig, dev, ("half", "tiles"), ref, monkeypatch, capfd, n, 1)
    rig.close()


def test_stale_summary(gpu, scenes, refs, monkeypatch, capfd):
    """A pin again with other contents: the summary follows the contents, never the previous pin."""
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    torch = rig.torch
    buf = torch.from_numpy(inputs["half"]).cuda()
    dev = {"half": buf, "rnd": buf}  # (one tensor: the address is the pin's key)
    pin(rig, buf)
    n = regular_count(capfd)
    n = check(rig, dev, ("half",), ref, monkeypatch, capfd, n, 1)
    buf.copy_(torch.from_numpy(inputs["rnd"]))
    pin(rig, buf)
    n = regular_count(capfd)
    n = check(rig, dev, ("rnd",), ref, monkeypatch, capfd, n, 0)
    # ... and with no synchronisation between the pin and the trace: whatever the launch finds, unknown
    # or known, it is never the previous contents' "regular".
    buf.copy_(torch.from_numpy(inputs["half"]))
    pin(rig, buf)
    buf.copy_(torch.from_numpy(inputs["rnd"]))
    rig.scene.pin_offsets(buf, rig.stream)
    got = launch(rig, [buf])
    assert same(got[0], ref["rnd"])
    assert regular_count(capfd) == n
    buf.copy_(torch.from_numpy(inputs["half"]))
    pin(rig, buf)
    n = regular_count(capfd)
    check(rig, dev, ("half",), ref, monkeypatch, capfd, n, 1)
    rig.scene.unpin_offsets(buf)
    rig.close()


@pytest.mark.parametrize("form", ["stream", "indexed"])
def test_list_overflow(gpu, scenes, refs, monkeypatch, capfd, form):
    """Lists overflowed by SRT_CULL_BIN_CAP=8: those tiles' descriptors say FULL and are not empty, so
    they stay list blocks and stream every record inside the regular kernel (its first copy of the
    body; only a sweep block's second copy is gone): the launch is regular, the bits are the same."""
    monkeypatch.setenv("SRT_CULL_BIN_CAP", "8")
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device(rig, inputs, ("half", "tiles"))
    for t in dev.values():
        pin(rig, t)
    n = regular_count(capfd)
    for names in (("half",), ("tiles", "half")):
        n = check(rig, dev, names, ref, monkeypatch, capfd, n, 1)
    rig.close()


def test_errors(gpu, scenes, refs, monkeypatch):
    """SRT_TRACE_POS=junk is an error, pinned frames or none; the switch is read per call."""
    import simpleraytracer_amd as srt

    inputs, ref = refs
    rig = Rig(scenes["soup2k"], W, H)
    dev = device(rig, inputs, ("half",))
    monkeypatch.setenv("SRT_TRACE_POS", "junk")
    with pytest.raises(srt.SrtError, match="SRT_TRACE_POS"):
        launch(rig, [dev["half"]])
    pin(rig, dev["half"])
    with pytest.raises(srt.SrtError, match="SRT_TRACE_POS"):
        launch(rig, [dev["half"]])
    monkeypatch.setenv("SRT_TRACE_POS", "")
    assert same(launch(rig, [dev["half"]])[0], ref["half"])
    rig.close()
