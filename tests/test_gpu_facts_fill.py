"""The fill of the statically empty tiles from the tile-facts launch (render.h CullSetup::empty_map,
facts_fill; env SRT_EMPTY_FILL=facts|sweep): on the shared setup the facts kernel (one wave per tile)
stores the misses of every tile the setup's map calls empty and whose offsets are valid in the frame;
the trace's sweep blocks then store nothing and only trace the invalid ones. With SRT_EMPTY_FILL=sweep
(the default) the sweep blocks fill, with SRT_EMPTY_SWEEP=0 one block per empty descriptor does. Every
pixel has one writer in each setting, and the three settings give the same frame.

Every comparison is bit for bit on the uint32 view against the `lds` brute-force variant of the same
library, on a scene object of its own. The outputs are prefilled with NaN (RGBA) and -7 (ids), so a
pixel nobody wrote fails; the counters under SRT_SETUP_LOG=1 (empty_descs, sweep_blocks,
facts_fill_frames) tell which setting a launch ran in and that the scene had empty tiles at all.

Shapes (tiles are 64 x 16): 200 x 72 -- 4 x 5 tiles, a last column of 8 pixels (the 8-B load path) and
a last tile row of 8 rows --, 1100 x 40 -- sky over more than two sweep groups of 16 --, 333 x 170 -- an
odd width: every tile on the 8-B load path. Scenes and inputs are test_gpu_empty_sweep's.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import test_gpu_empty_sweep as es
from scenefile import write_custom_scene
from test_gpu_empty_sweep import DEFAULT_GROUP, Rig, ids_of, lds_refs, make_inputs, same

pytestmark = pytest.mark.gpu

W, H = es.W, es.H        # 200 x 72
WW, WH = es.WW, es.WH    # 1100 x 40
W2, H2 = es.W2, es.H2    # 333 x 170
MODES = ("facts", "sweep", "off")
INPUTS = ("half", "rnd", "far", "nan", "above", "below")
EIGHT = ("half", "above", "nan", "rnd", "below", "far", "rnd2", "half")
NINE = ("half", "rnd", "far", "nan", "above", "below", "rnd2", "half", "nan")

STATS = re.compile(es.STATS.pattern + r" facts_fill_frames (\d+) lean_facts_frames (\d+)")
NAMES = es.NAMES + ("facts", "lean")
# The facts kernel each setting runs with (SRT_FACTS_KERNEL): the fill is the lean kernel's; `sweep` runs
# the lean kernel without the fill, `off` the block kernel. test_gpu_empty_sweep runs `auto`.
KERNEL = {"facts": "auto", "sweep": "lean", "off": "block"}


def all_stats(capfd):
    last = {}
    for m in STATS.finditer(capfd.readouterr().err):
        last[m.group(1)] = dict(zip(NAMES, (int(v) for v in m.groups()[1:])))
    assert last, "no setup counters with facts_fill_frames on stderr"
    return list(last.values())


def stats(capfd):
    every = all_stats(capfd)
    assert len(every) == 1
    return every[0]


def set_mode(monkeypatch, mode):
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    for name in ("SRT_SETUP", "SRT_EMPTY_GROUP", "SRT_EMPTY_FILL"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SRT_EMPTY_SWEEP", "0" if mode == "off" else "1")
    if mode != "off":
        monkeypatch.setenv("SRT_EMPTY_FILL", mode)
    monkeypatch.setenv("SRT_FACTS_KERNEL", KERNEL[mode])


def check_counters(s, mode, frames, sky):
    """Every frame on the shared setup; the sweep's grid is the same in both fill modes; the facts
    launch was asked to fill exactly the frames traced under `facts`."""
    assert (s["shared"], s["per_frame"]) == (frames, 0), s
    assert s["sweep"] == (0 if mode == "off" else -(-s["empty"] // DEFAULT_GROUP)), (mode, s)
    assert s["facts"] == (frames if mode == "facts" else 0), (mode, s)
    assert s["lean"] == (0 if mode == "off" else frames), (mode, s)
    if sky:
        assert s["empty"] > 0, s
    elif sky is not None:
        assert s["empty"] == 0, s


def cluster_scene(tmp_path_factory):
    """Small triangles in the lower left and nothing else: sky elsewhere at every size (no large list)."""
    rng = np.random.default_rng(5)
    tris = [list((rng.uniform([-0.9, -0.7, 3.0], [-0.2, -0.1, 5.0]) + rng.uniform(-0.08, 0.08, (3, 3))).ravel())
            for _ in range(150)]
    return write_custom_scene(tmp_path_factory.mktemp("cluster") / "cluster.srt", tris,
                              rng.uniform(0.2, 1.0, (len(tris), 3)))


class CameraRig(Rig):
    """A Rig whose scene is created under another camera than the file's."""

    def __init__(self, path, w, h, camera):
        import torch

        import simpleraytracer_amd as srt

        self.torch = torch
        self.scene = srt.DeviceScene(path, 0, camera=camera)
        self.stream = torch.cuda.current_stream()
        self.prepare(w, h)


@pytest.fixture(scope="module")
def cases(scenes, tmp_path_factory):
    """Per case: path, frame size, inputs and their brute-force frames (computed once, never changed)."""
    nasty = es.nasty_scene(tmp_path_factory)
    cluster = cluster_scene(tmp_path_factory)
    out = {}
    for name, path, w, h in (("sky", nasty, W, H), ("soup2k", scenes["soup2k"], W, H), ("wide", nasty, WW, WH),
                             ("odd", cluster, W2, H2)):
        inputs = make_inputs(w, h)
        out[name] = (path, w, h, inputs, lds_refs(path, w, h, inputs))
    for name in ("sky", "wide", "odd"):
        assert (out[name][4]["half"][..., 3] == -1).mean() > 0.2, name  # sky
    return out


SKY = {"sky": True, "soup2k": None, "wide": True, "odd": True}


@pytest.mark.parametrize("name", ["sky", "soup2k", "wide", "odd"])
def test_three_settings_agree(gpu, cases, monkeypatch, capfd, name):
    """Single frames and one 8-frame launch with a different input per frame (kernel arguments), as
    RGBA and as hit ids. `far`: every tile invalid, the facts launch fills nothing and the sweep blocks
    trace all; `nan`, `above`, `below`: filled and traced tiles share a group."""
    path, w, h, inputs, refs = cases[name]
    got = {}
    for mode in MODES:
        set_mode(monkeypatch, mode)
        rig = Rig(path, w, h)
        rgba = {k: rig.trace(inputs[k]) for k in INPUTS}
        ids = {k: rig.trace_ids(inputs[k]) for k in INPUTS}
        s = stats(capfd)
        assert s["builds"] == 1
        check_counters(s, mode, 2 * len(INPUTS), SKY[name])
        if name == "wide":
            assert s["empty"] >= 2 * DEFAULT_GROUP + 1, s
        batch = rig.trace_batch([inputs[k] for k in EIGHT])
        batch_ids = rig.trace_batch([inputs[k] for k in EIGHT], ids=True)
        check_counters(stats(capfd), mode, 2 * len(INPUTS) + 2 * len(EIGHT), SKY[name])
        rig.close()
        got[mode] = (rgba, ids, batch, batch_ids)
    for mode in MODES:
        rgba, ids, batch, batch_ids = got[mode]
        for k in INPUTS:
            assert same(rgba[k], refs[k]), (mode, k)
            assert np.array_equal(ids[k], ids_of(refs[k])), (mode, "ids", k)
        for i, k in enumerate(EIGHT):
            assert same(batch[i], refs[k]), (mode, "batch", i, k)
            assert np.array_equal(batch_ids[i], ids_of(refs[k])), (mode, "batch ids", i, k)


@pytest.mark.parametrize("name", ["sky", "odd"])
def test_nine_frame_launch(gpu, cases, monkeypatch, capfd, name):
    """Launches of 9 frames, RGBA: more than the kernel arguments hold, so the facts kernel and the
    trace read each frame's parameters, the map and the switch among them, from the device table.
    Python's batch entry takes 8 frames at most; an engine without an exchange traces its launches
    straight to RGBA through the same call. (Hit ids in a 9-frame launch: no Python entry reaches
    them; the packed ids below go through the table too.)"""
    from simpleraytracer_amd.engine import FrameEngine

    path, w, h, inputs, refs = cases[name]
    for mode in MODES:
        set_mode(monkeypatch, mode)
        with FrameEngine(path, w, h, devices=[0], batch=9, launch=9, queues=2) as e:
            e.set_inputs(np.stack([inputs[k] for k in NINE]))
            e.run(2)
            for f in range(18):
                assert same(e.read_frame(f), refs[NINE[f % 9]]), (mode, f)
        check_engine_counters(all_stats(capfd), mode, 18)


def check_engine_counters(every, mode, frames):
    assert sum(s["shared"] for s in every) >= frames and all(s["per_frame"] == 0 for s in every), every
    for s in every:
        assert s["empty"] > 0 and s["sweep"] == (0 if mode == "off" else -(-s["empty"] // DEFAULT_GROUP)), (mode, s)
        assert s["facts"] == (s["shared"] if mode == "facts" else 0), (mode, s)
        assert s["lean"] == (0 if mode == "off" else s["shared"]), (mode, s)


def deep_scene(tmp_path_factory):
    """The nasty scene behind 66 000 degenerate triangles (disabled records: they reach no tile): the
    visible ids lie above 65 535, so the packed ids have bit planes beside the u16 plane."""
    from scenefile import read_scene

    tris = read_scene(es.nasty_scene(tmp_path_factory))[2]
    pad = np.tile(np.array([0.3, 0.2, 4.0] * 3, np.float32), (66_000, 1))
    allv = np.concatenate([pad, tris])
    albedo = np.random.default_rng(8).uniform(0.2, 1.0, (len(allv), 3))
    return write_custom_scene(tmp_path_factory.mktemp("deep") / "deep.srt", allv, albedo)


@pytest.mark.parametrize("frames", [8, 9], ids=["args", "table"])
def test_packed_ids_through_the_exchange_engine(gpu, tmp_path_factory, monkeypatch, capfd, frames):
    """Packed ids (render.h PackedIds) at 200 x 72: an engine over a one-rank RCCL communicator traces
    whole frames on the shared setup into packed ids -- the u16 plane, the bit planes (ids above
    65 535), the tile's offset entry -- and the compositor shades them. `half`: filled tiles whose
    offset entry is (ox, oy); `rnd`: filled tiles with irregular offsets, entry NaN; `far`, `below`,
    `nan`: tiles the sweep blocks trace. 8 frames per launch: kernel arguments; 9: the table.
    What this verifies of a filled tile is its u16 plane and bit-plane stores. Its offset entry is
    written but not observable here: the deferred shading reads a tile's entry only for hits, a
    filled tile has none, and no Python entry exposes the packed buffer. The entry's store is the one
    function the sweep fill and the trace body call too (StorePackedTileOffset)."""
    from simpleraytracer_amd.engine import FrameEngine

    path = deep_scene(tmp_path_factory)
    inputs = make_inputs(W, H)
    names = EIGHT if frames == 8 else NINE
    refs = lds_refs(path, W, H, {k: inputs[k] for k in set(names)})
    assert (refs["half"][..., 3] == -1).mean() > 0.2 and refs["half"][..., 3].max() > 65_535
    for mode in MODES:
        set_mode(monkeypatch, mode)
        with FrameEngine(path, W, H, devices=[0], batch=frames, launch=frames, queues=2, rccl_self=True) as e:
            assert e.info()["rccl"]
            e.set_inputs(np.stack([inputs[k] for k in names]))
            e.run(2)
            for f in range(2 * frames):
                assert same(e.read_frame(f), refs[names[f % frames]]), (mode, f)
        check_engine_counters(all_stats(capfd), mode, 2 * frames)


def test_offsets_eight_byte_aligned(gpu, cases, monkeypatch, capfd):
    """An offsets tensor one float2 into a larger buffer: 8-B but not 16-B aligned, so the even-width
    frame's whole tiles take the 8-B load path too."""
    import torch

    path, w, h, inputs, refs = cases["sky"]
    for mode in ("facts", "sweep"):
        set_mode(monkeypatch, mode)
        rig = Rig(path, w, h)
        for k in ("rnd", "below", "half"):
            buf = torch.zeros(h * w * 2 + 2, dtype=torch.float32, device="cuda")
            view = buf[2:].view(h, w, 2)
            view.copy_(torch.from_numpy(inputs[k]))
            assert view.data_ptr() % 16 == 8 and view.is_contiguous()
            out = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
            rig.scene.trace(view, out, 0, h, variant="cull", stream=rig.stream)
            torch.cuda.synchronize()
            assert same(out.cpu().numpy(), refs[k]), (mode, k)
        check_counters(stats(capfd), mode, 3, True)
        rig.close()


def test_map_follows_the_prepared_size(gpu, cases, monkeypatch, capfd):
    """200 x 72, 1100 x 40 and back on one scene: every build writes its own plan's map."""
    path, w, h, inputs, refs = cases["sky"]
    _, ww, wh, winputs, wrefs = cases["wide"]
    set_mode(monkeypatch, "facts")
    rig = Rig(path, w, h)
    assert same(rig.trace(inputs["rnd"]), refs["rnd"])
    a = stats(capfd)
    rig.prepare(ww, wh)
    for k in ("rnd", "below"):
        assert same(rig.trace(winputs[k]), wrefs[k]), k
    b = stats(capfd)
    rig.prepare(w, h)
    for k in ("below", "half"):
        assert same(rig.trace(inputs[k]), refs[k]), k
    c = stats(capfd)
    check_counters(c, "facts", 5, True)
    assert (a["builds"], b["builds"], c["builds"]) == (1, 2, 3)
    assert b["empty"] > a["empty"] == c["empty"] > 0
    rig.close()


def test_map_follows_a_camera_move(gpu, cases, monkeypatch, capfd):
    """The motion family's entry (DeviceScene.set_camera): the camera turns so that geometry enters
    tiles that were sky, and turns back, so that those tiles are sky again. A stale map shows on the
    way back: the sweep block skips a tile the facts wave no longer fills, and nobody writes it."""
    path, w, h, inputs, refs = cases["sky"]
    turned = (0.0, 0.0, 0.0, -3.0, -2.0, 4.0, 0.0, 1.0, 0.0, 60.0)
    fresh = CameraRig(path, w, h, turned)
    after = {k: fresh.trace(inputs[k], variant="lds") for k in ("rnd", "below")}
    fresh.close()
    ref_rig = Rig(path, w, h)
    home = tuple(ref_rig.scene.camera)
    ref_rig.close()
    # Conditions of the case: whole tiles that are sky at home and have hits when turned (entered on
    # the way there, vacated on the way back), and whole tiles for which it is the other way round.
    th, tw = -(-h // 16), -(-w // 64)

    def tiles(sky_in, hits_in):
        return [(r, c) for r in range(th) for c in range(tw)
                if (sky_in[16 * r:16 * r + 16, 64 * c:64 * c + 64, 3] == -1).all()
                and (hits_in[16 * r:16 * r + 16, 64 * c:64 * c + 64, 3] >= 0).any()]

    assert tiles(refs["rnd"], after["rnd"]), "no tile that is sky at home has geometry when turned"
    assert tiles(after["rnd"], refs["rnd"]), "no tile that has geometry at home is sky when turned"
    for mode in ("facts", "sweep"):
        set_mode(monkeypatch, mode)
        rig = Rig(path, w, h)
        assert same(rig.trace(inputs["rnd"]), refs["rnd"]), mode
        rig.scene.set_camera(turned, stream=rig.stream)
        for k in ("rnd", "below"):
            assert same(rig.trace(inputs[k]), after[k]), (mode, k)
        rig.scene.set_camera(home, stream=rig.stream)
        for k in ("rnd", "below"):
            assert same(rig.trace(inputs[k]), refs[k]), (mode, "back", k)
        s = stats(capfd)
        assert s["builds"] == 3
        check_counters(s, mode, 5, True)
        rig.close()


def test_cornell_has_nothing_to_fill(gpu, scenes, monkeypatch, capfd):
    """Cornell at 192 x 108: no descriptor is empty, so neither launch fills; the counter still says
    which launch was asked to."""
    w, h = 192, 108
    inputs = {"half": np.full((h, w, 2), 0.5, np.float32),
              "rnd": np.random.default_rng(9).random((h, w, 2), dtype=np.float32)}
    refs = lds_refs(scenes["cornell"], w, h, inputs)
    for mode in MODES:
        set_mode(monkeypatch, mode)
        rig = Rig(scenes["cornell"], w, h)
        for k in ("half", "rnd", "half"):
            assert same(rig.trace(inputs[k]), refs[k]), (mode, k)
        s = stats(capfd)
        check_counters(s, mode, 3, False)
        assert s["sweep"] == 0, s
        rig.close()


def test_default_is_the_sweep_fill(gpu, cases, monkeypatch, capfd):
    """Unset, the switch means `sweep` (the facts fill measured slower on the headline); the facts
    kernel is the same one-wave-per-tile kernel either way."""
    path, w, h, inputs, refs = cases["sky"]
    set_mode(monkeypatch, "sweep")
    monkeypatch.delenv("SRT_EMPTY_FILL")
    rig = Rig(path, w, h)
    for k in ("rnd", "below"):
        assert same(rig.trace(inputs[k]), refs[k]), k
    check_counters(stats(capfd), "sweep", 2, True)
    rig.close()


def test_auto_picks_the_kernel_by_offsets_reuse(gpu, cases, monkeypatch, capfd):
    """SRT_FACTS_KERNEL unset: a launch whose frames share an offsets buffer runs the lean kernel, a
    single frame and a launch of frames with offsets of their own the block kernel; the same frames."""
    import torch

    path, w, h, inputs, refs = cases["sky"]
    set_mode(monkeypatch, "sweep")
    monkeypatch.delenv("SRT_FACTS_KERNEL")
    rig = Rig(path, w, h)
    assert same(rig.trace(inputs["below"]), refs["below"])
    assert stats(capfd)["lean"] == 0
    for k, got in zip(EIGHT, rig.trace_batch([inputs[k] for k in EIGHT])):
        assert same(got, refs[k]), k
    assert stats(capfd)["lean"] == 0
    off = rig._up(inputs["nan"])
    outs = [torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
    rig.scene.trace_batch([off] * 4, outs, 0, h, variant="cull", stream=rig.stream)
    torch.cuda.synchronize()
    for o in outs:
        assert same(o.cpu().numpy(), refs["nan"])
    s = stats(capfd)
    assert (s["lean"], s["shared"], s["facts"]) == (4, 13, 0), s
    rig.close()


def test_junk_fill_switch(gpu, cases, monkeypatch):
    import simpleraytracer_amd as srt

    path, w, h, inputs, refs = cases["sky"]
    rig = Rig(path, w, h)
    for var, junk in (("SRT_EMPTY_FILL", "yes"), ("SRT_EMPTY_FILL", "1"), ("SRT_EMPTY_FILL", "Facts"),
                      ("SRT_EMPTY_FILL", "sweep "), ("SRT_FACTS_KERNEL", "fat"), ("SRT_FACTS_KERNEL", "1")):
        monkeypatch.setenv(var, junk)
        with pytest.raises(srt.SrtError, match=var):
            rig.trace(inputs["half"])
        monkeypatch.delenv(var)
    assert same(rig.trace(inputs["half"]), refs["half"])
    rig.close()
