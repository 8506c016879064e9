"""Triangle counts on the device: tests/count_cases.py's scenes N(n) -- n on and next to every
boundary of the library's blocking (8 and its powers: BVH leaves, nodes and levels; 256: record,
extent and shading-table blocks, edge tiles; 4 096: the padded count, the cull step, the minimum list
capacity; 65 536 and 131 072: the bit planes of the packed ids), with sentinels at the tails of the
spatial order, and the dead-tail variants -- through the spatial order, every trace variant, the
cull's set-ups, point queries, layers, surface attributes, deferred shading and the packed-id
exchange.

Nothing here has a tolerance of its own: ids and t are compared on the bits, RGB at the project's
1e-5 against the oracle (test_gpu_parity.assert_parity), the normal as in gbuffer_cases. The CPU
backend equals the oracle on every case and the guards hold (test_count_host.py): a mismatch here is
a device-side bug. Frames are 256 x 144, and 200 x 72 where a test says so.
"""
from __future__ import annotations

import numpy as np
import pytest

import count_cases as cc
import gbuffer_cases as gc
import layers_cases as lc
import query_cases as qc
import test_gpu_gbuffer
import test_gpu_layers
import test_gpu_query
from test_gpu_parity import VARIANTS, assert_parity, torch_render

pytestmark = pytest.mark.gpu

W, H = cc.W, cc.H
BANDS = [37, 1, 50, 56]
SMALL_AND_DEAD = cc.SMALL_NAMES + cc.DEAD_NAMES
SETUP_NAMES = SMALL_AND_DEAD + (cc.name_of(65536),)
SETUPS = {
    "stored": ("SRT_TRACE_RECORDS", "stored"),
    "recompute": ("SRT_TRACE_RECORDS", "recompute"),
    "indexed": ("SRT_TRACE_STREAM", "0"),
    "frame_setup": ("SRT_SETUP", "frame"),
    "no_bins": ("SRT_CULL_BIN", "0"),
    "cap8": ("SRT_CULL_BIN_CAP", "8"),  # every tile streams through n_pad: the pad records are visited
    "chunk64": ("SRT_CULL_CHUNK", "64"),
    "no_sweep": ("SRT_EMPTY_SWEEP", "0"),
}
ENV = ("SRT_SETUP", "SRT_SETUP_LOG", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_CULL_CHUNK", "SRT_CULL_CHUNKS",
       "SRT_CULL_SPLIT", "SRT_TRACE_RECORDS", "SRT_TRACE_STREAM", "SRT_EMPTY_SWEEP", "SRT_EMPTY_GROUP", "SRT_WORK_PLAN",
       "SRT_TRACE_VARIANT", "SRT_EXCHANGE_IDS", "SRT_GATHER", "SRT_BAND_ROWS", "ML_VISIBLE_DEVICES")


@pytest.fixture(autouse=True)
def default_env(gpu, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def same_bits(a, b):
    return np.array_equal(cc.bits(a), cc.bits(b))


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_spatial_order(name):
    """The device's order (Morton keys, the radix sort at this size) is the restated one entry for
    entry: the device's tails are the tails the guards reasoned about."""
    import simpleraytracer_amd as srt

    c = cc.case(name)
    scene = srt.DeviceScene(c.path, 0)
    order, _ = scene.spatial_order()
    scene.close()
    assert order.shape == (c.n,)
    bad = np.flatnonzero(order != c.order)
    assert bad.size == 0, f"{bad.size} entries differ, first at position {bad[0]}: {order[bad[0]]} != {c.order[bad[0]]}"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_variants(name, variant):
    """Random and uniform offsets against the oracle; the random frame as uneven bands bit for bit; the
    small counts also at 200 x 72 (a partial tile column and row)."""
    c = cc.case(name)
    for kind in ("rnd", "half"):
        got = torch_render(c.path, W, H, cc.offsets(W, H, kind), variant=variant)
        assert_parity(got, cc.frame(name, kind))
        if kind == "rnd":
            assert sum(BANDS) == H
            banded = torch_render(c.path, W, H, cc.offsets(W, H), variant=variant, bands=BANDS)
            assert same_bits(banded, got), "the banded frame differs"
    if name in SMALL_AND_DEAD:
        for kind in ("rnd", "half"):
            got = torch_render(c.path, cc.ODD_W, cc.ODD_H, cc.offsets(cc.ODD_W, cc.ODD_H, kind), variant=variant)
            assert_parity(got, cc.frame(name, kind, cc.ODD_W, cc.ODD_H))


@pytest.mark.parametrize("setup", SETUPS)
@pytest.mark.parametrize("name", SETUP_NAMES)
def test_cull_setups(monkeypatch, name, setup):
    """The set-ups that change which tail the cull variant reads, each against the oracle's frames."""
    c = cc.case(name)
    monkeypatch.setenv(*SETUPS[setup])
    for kind in ("rnd", "half"):
        assert_parity(torch_render(c.path, W, H, cc.offsets(W, H, kind), variant="cull"), cc.frame(name, kind))


@pytest.mark.parametrize("name", SETUP_NAMES)
def test_cull_batch_of_three(name):
    """One trace_batch of three frames with different offsets: each the oracle's."""
    import torch

    import simpleraytracer_amd as srt

    c = cc.case(name)
    kinds = ("rnd", "half", "rnd2")
    scene = srt.DeviceScene(c.path, 0)
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    off = [torch.full((H, W, 2), 0.5, dtype=torch.float32, device="cuda") if k == "half" else
           torch.from_numpy(cc.offsets(W, H, k)).cuda() for k in kinds]
    out = [torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in kinds]
    scene.trace_batch(off, out, 0, H, variant="cull", stream=stream)
    torch.cuda.synchronize()
    frames = [o.cpu().numpy() for o in out]
    scene.close()
    for k, got in zip(kinds, frames):
        assert_parity(got, cc.frame(name, k))


@pytest.mark.parametrize("cap", ["", "8"], ids=["default", "cap8"])
@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_query_and_layers(monkeypatch, name, cap):
    """scene.query and scene.layers (K = 4) at the mixed positions, the sentinels' centroids and a
    pixel each sentinel wins: exact against the oracle; with the lists capped at 8 entries the
    overflowed tiles stream every record through n_pad."""
    if cap:
        monkeypatch.setenv("SRT_CULL_BIN_CAP", cap)
    c = cc.case(name)
    pos, want_ids, want_t = cc.answers(name)
    _, l_ids, l_t = cc.layers(name)
    inside = qc.in_range(pos)
    rig = test_gpu_query.Rig(c.path, W, H)
    ids, t, how = rig.query(pos)
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    rig = test_gpu_layers.Rig(c.path, W, H)
    ids4, t4, how4 = rig.layers(pos, cc.LAYERS)
    rig.close()
    lc.assert_same(ids4, t4, l_ids, l_t)
    for h in (how, how4):
        assert np.all(h[~inside] == 1)
        if not cap:
            assert np.all(h[inside] == 0)


@pytest.mark.parametrize("cap", ["", "8"], ids=["default", "cap8"])
@pytest.mark.parametrize("name", cc.SHADOW_NAMES)
def test_shadow_families(monkeypatch, name, cap):
    """scene.shadow under L1, omni_shadow under the point light at L1's eye and scene.light under both
    spot lights and the point light, whole frame, ids the oracle's: every class byte, the face plane
    and the RGBA equal the host paths' on the bits (count_cases.shadow_answers, whose guards say what
    the light orders' tails decide; n9 and n257 run without the knock-out guard: count_cases.KNOCK_OUT).
    With the lists capped at 8 entries the overflowed tiles of every light frame stream through n_pad."""
    import torch

    import simpleraytracer_amd as srt

    if cap:
        monkeypatch.setenv("SRT_CULL_BIN_CAP", cap)
    c = cc.case(name)
    want = cc.shadow_answers(name)
    stream = torch.cuda.current_stream()
    view = srt.DeviceScene(c.path, 0)
    view.prepare(W, H, stream)
    spots = [srt.DeviceScene(c.path, 0, camera=cam) for cam in (cc.L1, cc.L2)]
    for s in spots:
        s.prepare(W, H, stream)
    point = srt.OmniLight(c.path, 0, cc.POINT_ORIGIN)
    point.prepare(cc.FACE_SIZE, stream)
    off = torch.from_numpy(cc.offsets(W, H)).cuda()
    ids = torch.from_numpy(np.array(cc.frame_ids(name))).cuda()
    mask, omask, face = (torch.full((H, W), 9, dtype=torch.uint8, device="cuda") for _ in range(3))
    rgba, orgba, lrgba = (torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3))
    classes = torch.full((3, H, W), 9, dtype=torch.uint8, device="cuda")
    view.shadow(spots[0], off, ids, mask, rgba, dim=cc.SHADOW_DIM, stream=stream)
    view.omni_shadow(point, off, ids, omask, face, orgba, dim=cc.SHADOW_DIM, stream=stream)
    lights = [srt.SpotLight(spots[0], cc.LIGHT_COLORS[0], cc.LIGHT_FALLOFF[0]),
              srt.SpotLight(spots[1], cc.LIGHT_COLORS[1], cc.LIGHT_FALLOFF[1]),
              srt.PointLight(point, cc.LIGHT_COLORS[2], cc.LIGHT_FALLOFF[2])]
    view.light(lights, off, ids, lrgba, ambient=cc.AMBIENT, classes=classes, stream=stream)
    torch.cuda.synchronize()
    got = [a.cpu().numpy() for a in (mask, rgba, omask, face, orgba, lrgba, classes)]
    point.close()
    for s in spots:
        s.close()
    view.close()
    names = ("shadow mask", "shadow rgba", "omni mask", "omni face", "omni rgba", "lighting rgba", "lighting classes")
    for what, g, w in zip(names, got, (*want.spot, *want.omni, *want.lighting)):
        if g.dtype == np.uint8:
            assert w.dtype == np.uint8 and np.array_equal(g, w), f"{what}: {int((g != w).sum())} bytes differ"
        else:
            lc.same_bits(what, g, w)


@pytest.mark.parametrize("name", SMALL_AND_DEAD)
def test_layer_frame_odd(name):
    """scene.layer_frame at 200 x 72 equals the peeled oracle, every pixel answered from the lists."""
    c = cc.case(name)
    want_ids, want_t = cc.odd_layers(name)
    rig = test_gpu_layers.Rig(c.path, cc.ODD_W, cc.ODD_H)
    ids, t, how = rig.layer_frame(cc.offsets(cc.ODD_W, cc.ODD_H), cc.LAYERS)
    rig.close()
    lc.assert_same(ids, t, want_ids, want_t)
    assert np.all(how == 0)


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_attributes_at_the_sentinels(name):
    """scene.attributes at the sentinels' positions (id n - 1 reads the last shading-table entry)
    and at 300 of the mixed positions, misses among them: test_gpu_gbuffer's checks against the
    oracle, and attributes_host's planes -- depth, barycentrics and albedo on the bits, the normal
    within 2 x 2^-22 (each side is within 2^-22 of the float64 normal)."""
    import simpleraytracer_amd.device as device

    c = cc.case(name)
    pos, ids, t = cc.answers(name)
    m = 2 * len(c.sentinels)
    pick = np.r_[0:300, len(pos) - m:len(pos)]
    pos, ids, t = pos[pick], ids[pick], t[pick]
    assert set(c.sentinels) <= set(ids.tolist()) and (ids < 0).any()
    exp = gc.expected(c.path, W, H, pos, ids)
    rig = test_gpu_gbuffer.Rig(c.path, W, H)
    got = rig.attributes(pos, ids)
    rig.close()
    gc.check_planes(exp, **got)
    gc.check_misses(ids, exp.n, exp.background, **got)
    lc.same_bits("depth against the oracle's t", got["depth"], t)
    depth, bary, normal, albedo = device.attributes_host(c.path, W, H, pos, ids)
    lc.same_bits("depth against the host", got["depth"], depth)
    lc.same_bits("bary against the host", got["bary"], bary)
    lc.same_bits("albedo against the host", got["albedo"], albedo)
    assert float(np.abs(got["normal"] - normal).max()) <= 2 * gc.NORMAL_TOL


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_deferred_shading(name):
    """trace_ids then shade equals the fused trace bit for bit in every variant; the ids are the
    oracle's, id n - 1 among them."""
    import torch

    import simpleraytracer_amd as srt

    c = cc.case(name)
    want = cc.frame(name)
    assert (want[..., 3] == c.live - 1).any()
    scene = srt.DeviceScene(c.path, 0)
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    off = torch.from_numpy(cc.offsets(W, H)).cuda()
    for variant in VARIANTS:
        fused = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        ids = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
        rgba = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        scene.trace(off, fused, 0, H, variant=variant, stream=stream)
        scene.trace_ids(off, ids, 0, H, variant=variant, stream=stream)
        scene.shade(off, ids, rgba, 0, H, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy().astype(np.float32), want[..., 3]), variant
        assert same_bits(rgba.cpu().numpy(), fused.cpu().numpy()), variant
    scene.close()


@pytest.mark.parametrize("ids32", [False, True], ids=["packed", "int32"])
@pytest.mark.parametrize("n", cc.PLANE_COUNTS)
def test_packed_ids_at_the_plane_boundaries(monkeypatch, n, ids32):
    """n = 65 535 packs in 16 bits, 65 536 to 131 071 need one bit plane, 131 072 two: id n - 1 (low
    bits all ones at 65 536 and 131 072, where only the planes tell it from a miss) and misses in one
    tile row, through the fake-device exchange (P = 2 and 3), the one-rank RCCL exchange and the
    mlInfer gather, packed and as int32: the one-device frame bit for bit, which is the oracle's.
    The exchanged bytes are those of the packed layout with 0, 1, 1, 1 and 2 planes."""
    import simpleraytracer_amd as srt
    from simpleraytracer_amd.engine import FrameEngine

    name = cc.name_of(n)
    c = cc.case(name)
    inputs = np.stack([cc.offsets(W, H), cc.offsets(W, H, "rnd2")])
    inputs[1, :48] = 0.5  # regular tiles (their offset travels with the packed ids): three tile rows,
    inputs[1, 48:, 128:192] = 0.25  # and one tile column below them
    refs = [torch_render(c.path, W, H, inputs[k]) for k in range(2)]
    assert_parity(refs[0], cc.frame(name))
    for ref in refs:
        tile_rows = ref[..., 3].reshape(H // 16, 16 * W)
        assert ((tile_rows == n - 1).any(axis=1) & (tile_rows == -1).any(axis=1)).any(), \
            "no tile row holds both id n - 1 and a miss"
    if ids32:
        monkeypatch.setenv("SRT_EXCHANGE_IDS", "32")
    for kw in ({"devices": [0, 0]}, {"devices": [0, 0, 0]}, {"devices": [0], "rccl_self": True}):
        with FrameEngine(c.path, W, H, batch=6, queues=2, **kw) as e:
            info = e.info()
            e.set_inputs(np.concatenate([inputs] * 3))
            e.run(1)
            for k in range(6):
                assert same_bits(e.read_frame(k), refs[k % 2]), (kw, k)
        world = len(kw["devices"])
        if world > 1:  # bands of the 9 tile rows dealt round-robin: buffers of ceil(9 / P) tile rows
            rows = (9 + world - 1) // world * 16
            assert info["buffer_rows"] == rows
            band = rows * W * 4 if ids32 else cc.packed_band_bytes(cc.id_planes(n), rows, W)
            assert info["exchange_bytes_per_frame"] == (world - 1) * band, (kw, info)
    ref = srt.render(c.path, W, H, inputs[0])
    assert same_bits(ref, refs[0])
    monkeypatch.setenv("ML_VISIBLE_DEVICES", "0,0,0")
    assert same_bits(srt.render(c.path, W, H, inputs[0]), refs[0])
