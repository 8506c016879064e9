"""Coordinate range on the device: tests/scale_cases.py's scenes -- scene S times 2^k across and far
beyond the float screen-box solve's range [2^-40, 2^30], translated far from the origin, under a 1
degree view, and the cloud under telephoto, fisheye, strip-frame and rolled cameras -- through every
trace variant, the cull's modes, point queries, layers, the G-buffer, multi-sample frames, shadow
masks, the band engine and the spatial order.

Nothing here has a tolerance of its own: ids and t are compared on the bits, RGB at the project's
1e-5 against the oracle (test_gpu_parity.assert_parity). Power-of-two scaling is exact in every
expression involved (scale_cases), so a frame of S times 2^k also has the ids of the device's own
k = 0 frame and, for |k| <= 20, its RGB bits. The CPU backend equals the oracle on every case
(test_scale_host.py): a mismatch here is a device-side bug. Frames are 200 x 72 unless the case says
otherwise.
"""
from __future__ import annotations

import numpy as np
import pytest

import gbuffer_cases as gc
import layers_cases as lc
import query_cases as qc
import samples_cases as smp
import scale_cases as sc
import test_gpu_gbuffer
import test_gpu_layers
import test_gpu_query
import test_gpu_samples
import test_gpu_trace_stream as ts
from test_gpu_parity import VARIANTS, assert_parity, morton_order_numpy, torch_render

pytestmark = pytest.mark.gpu

W, H = sc.W, sc.H
SWEEP_KS = (-30, -21, -16, -15, 0, 14, 15, 16, 21, 30)
TRANSITION_KS = (-21, 15, 16, 30)
POINT_CASES = ("k-21", "k0", "k16", "k30", "tele2000", "fish179")
PLANE_KS = (-21, 16)
ORDER_KS = (-21, 16, 30)
ENGINE_CASES = ("k16", "k-21", "tele200", "fish179")
BANDS = {"wide": [3, 5], "wide4100": [1, 2], "tall": [777, 1223]}  # two uneven bands of the strip frames
ENV = ("SRT_SETUP", "SRT_SETUP_LOG", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_CULL_CHUNK", "SRT_CULL_CHUNKS",
       "SRT_CULL_SPLIT", "SRT_TRACE_RECORDS", "SRT_TRACE_STREAM")


@pytest.fixture(autouse=True)
def default_env(gpu, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def same_bits(a, b):
    return np.array_equal(sc.bits(a), sc.bits(b))


@pytest.fixture(scope="module")
def own_k0(gpu):
    """The device's own frame of S at k = 0 with the random offsets, per variant: read-only."""
    c = sc.case("k0")
    out = {v: torch_render(c.path, W, H, sc.offsets(W, H), variant=v) for v in VARIANTS}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("k", SWEEP_KS)
def test_scale_sweep(own_k0, k, variant):
    """S times 2^k: the oracle's frame; the ids of the device's own k = 0 frame, and its RGB bits
    while n . n stays in the float range (|k| <= 20)."""
    c = sc.case(sc.s_name(k))
    got = torch_render(c.path, W, H, sc.offsets(W, H), variant=variant)
    assert_parity(got, sc.frame(c.name))
    assert same_bits(got[..., 3], own_k0[variant][..., 3]), "ids differ from the device's own k = 0 frame"
    if abs(k) <= sc.RGB_EXACT_K:
        bad = np.argwhere(sc.bits(got[..., :3]) != sc.bits(own_k0[variant][..., :3]))
        assert bad.size == 0, (f"{len(bad)} RGB values differ from the device's own k = 0 frame, first at "
                               f"{tuple(bad[0])}: {got[tuple(bad[0])]!r} != {own_k0[variant][tuple(bad[0])]!r}")


@pytest.mark.parametrize("on", [True, False], ids=["stream", "indexed"])
@pytest.mark.parametrize("k", TRANSITION_KS)
def test_cull_record_stream_at_the_transitions(monkeypatch, capfd, k, on):
    """The shared setup's record stream on and off where the records change solve: the oracle's
    frame, and the counters say the frame took the path asked for."""
    c = sc.case(sc.s_name(k))
    ts.set_stream(monkeypatch, on)
    rig = ts.Rig(c.path, W, H)
    got = rig.trace(sc.offsets(W, H))
    s = ts.stats(capfd)
    rig.close()
    assert s["builds"] == 1
    ts.check_counters(s, on, 1)
    assert_parity(got, sc.frame(c.name))


@pytest.mark.parametrize("name,value", [("SRT_TRACE_RECORDS", "stored"), ("SRT_TRACE_RECORDS", "recompute"),
                                        ("SRT_CULL_BIN_CAP", "8"), ("SRT_SETUP", "frame")])
@pytest.mark.parametrize("k", TRANSITION_KS)
def test_cull_modes_at_the_transitions(monkeypatch, k, name, value):
    c = sc.case(sc.s_name(k))
    monkeypatch.setenv(name, value)
    for kind in ("rnd", "half"):
        off = sc.offsets(W, H) if kind == "rnd" else None
        assert_parity(torch_render(c.path, W, H, off, variant="cull"), sc.frame(c.name, kind))


@pytest.mark.parametrize("k", TRANSITION_KS)
def test_uneven_bands_at_the_transitions(k):
    """Row bands of 37, 1 and 34 rows: bit-equal to the whole frame, which is the oracle's."""
    c = sc.case(sc.s_name(k))
    whole = torch_render(c.path, W, H, sc.offsets(W, H), variant="cull")
    assert_parity(whole, sc.frame(c.name))
    banded = torch_render(c.path, W, H, sc.offsets(W, H), variant="cull", bands=[37, 1, 34])
    assert same_bits(banded, whole)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sc.CLOUD_NAMES + sc.EXTRA_NAMES)
def test_cameras(name, variant):
    """Telephoto, fisheye, strip frames, a rolled camera, a 1 degree view and far translations, with
    uniform 0.5 and random offsets; the strip frames also as two uneven bands."""
    c = sc.case(name)
    for kind in ("half", "rnd"):
        off = sc.offsets(c.w, c.h) if kind == "rnd" else None
        got = torch_render(c.path, c.w, c.h, off, variant=variant)
        assert_parity(got, sc.frame(name, kind))
    if name in BANDS:
        assert sum(BANDS[name]) == c.h
        banded = torch_render(c.path, c.w, c.h, off, variant=variant, bands=BANDS[name])
        assert same_bits(banded, got)


def report_how(what, how, inside):
    """`how` is 0 (answered from the tile's list) exactly for the positions in [0, 1]^2, as at scale 1
    (test_gpu_query.py): no case passes on a kernel that streams every record. Reported first."""
    print(f"{what}: {int((how[inside] == 0).sum())} of {int(inside.sum())} in-range positions answered from the lists, "
          f"{int((how[~inside] == 1).sum())} of {int((~inside).sum())} out-of-range ones streamed")
    assert inside.sum() >= 2000 and (~inside).sum() >= len(qc.OUT_OF_RANGE) ** 2
    assert np.array_equal(how, np.where(inside, 0, 1).astype(np.uint8))


@pytest.mark.parametrize("name", POINT_CASES)
def test_query_and_layers_at_the_mixed_positions(name):
    c = sc.case(name)
    pos, want_ids, want_t = sc.answers(name)
    _, l_ids, l_t = sc.layers(name)
    inside = qc.in_range(pos)
    rig = test_gpu_query.Rig(c.path, c.w, c.h)
    ids, t, how = rig.query(pos)
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    report_how(f"{name} query", how, inside)
    rig = test_gpu_layers.Rig(c.path, c.w, c.h)
    ids4, t4, how4 = rig.layers(pos, sc.LAYERS)
    rig.close()
    lc.assert_same(ids4, t4, l_ids, l_t)
    report_how(f"{name} layers", how4, inside)


@pytest.mark.parametrize("name", POINT_CASES)
def test_layer_frame_equals_the_peeled_oracle(name):
    c = sc.case(name)
    _, want_ids, want_t = sc.layers(name, "pixels")
    rig = test_gpu_layers.Rig(c.path, c.w, c.h)
    ids, t, how = rig.layer_frame(sc.offsets(c.w, c.h), sc.LAYERS)
    rig.close()
    lc.assert_same(ids, t, want_ids.reshape(-1, c.h, c.w), want_t.reshape(-1, c.h, c.w))
    print(f"{name} layer_frame: {int((how == 0).sum())} of {how.size} pixels answered from the lists")
    assert np.all(how == 0)


def gbuffer_planes(name):
    """(ids, planes) of the device's trace_ids and gbuffer of a case's frame with the random offsets."""
    c = sc.case(name)
    rig = test_gpu_gbuffer.Rig(c.path, c.w, c.h)
    ids = rig.trace(sc.offsets(c.w, c.h), ids=True)
    planes = rig.gbuffer(sc.offsets(c.w, c.h), ids)
    rig.close()
    return ids, planes


@pytest.fixture(scope="module")
def planes_k0(gpu):
    ids, planes = gbuffer_planes("k0")
    for a in (ids, *planes.values()):
        a.setflags(write=False)
    return ids, planes


@pytest.mark.parametrize("k", PLANE_KS)
def test_gbuffer_across_scale(planes_k0, k):
    """gbuffer_cases' checks against the oracle at k; depth is the device's own k = 0 depth times
    2^k, barycentrics, normal and albedo its k = 0 planes: bit for bit."""
    c = sc.case(sc.s_name(k))
    ids0, g0 = planes_k0
    ids, g = gbuffer_planes(c.name)
    want_ids = sc.frame_ids(c.name)
    assert np.array_equal(ids, want_ids) and np.array_equal(ids, ids0)
    exp = gc.expected(c.path, W, H, lc.pixel_positions(W, H, sc.offsets(W, H)), want_ids.reshape(-1))
    gc.check_planes(exp, **g)
    gc.check_misses(ids, exp.n, exp.background, **g)
    lc.same_bits("depth against k = 0", g["depth"], sc.scaled_t(g0["depth"], k))
    for plane in ("bary", "normal", "albedo"):
        lc.same_bits(f"{plane} against k = 0", g[plane], g0[plane])


@pytest.mark.parametrize("k", PLANE_KS)
def test_render_samples_across_scale(k):
    """S = 4 stratified samples: coverage exact, rgb within 1e-5 + S 2^-24 of the numpy resolve of
    the oracle's per-sample frames (samples_cases), the id planes the oracle's."""
    from oracle.srt_oracle import OracleScene
    from simpleraytracer_amd.samples import stratified_offsets

    c = sc.case(sc.s_name(k))
    off = stratified_offsets(W, H, 4, seed=17)
    o = OracleScene(c.path)
    frames = np.stack([o.render(W, H, off[s]) for s in range(4)])
    o.close()
    hits = (frames[..., 3] >= 0).sum(axis=0)
    assert ((hits > 0) & (hits < 4)).mean() >= 0.02  # pixels of partial coverage
    rig = test_gpu_samples.Rig(c.path, W, H)
    rgba, ids = rig.render_samples(off)
    rig.close()
    assert np.array_equal(ids.astype(np.float32), frames[..., 3])
    smp.check_against_oracle(f"render_samples S=4, k={k}", rgba, frames)


def device_shadow(k, bias):
    import torch

    import simpleraytracer_amd as srt

    c = sc.case(sc.s_name(k))
    stream = torch.cuda.current_stream()
    view, light = srt.DeviceScene(c.path, 0), srt.DeviceScene(c.path, 0, camera=sc.light_camera(k))
    view.prepare(W, H, stream)
    light.prepare(sc.LIGHT_W, sc.LIGHT_H, stream)
    off = torch.from_numpy(np.array(sc.offsets(W, H))).cuda()
    ids = torch.from_numpy(np.array(sc.frame_ids(c.name))).cuda()
    mask = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
    view.shadow(light, off, ids, mask, None, bias=bias, stream=stream)
    torch.cuda.synchronize()
    out = mask.cpu().numpy()
    view.close()
    light.close()
    return out


def host_shadow(k, bias):
    from simpleraytracer_amd import device

    c = sc.case(sc.s_name(k))
    return device.shadow_host(c.path, W, H, sc.light_camera(k), sc.LIGHT_W, sc.LIGHT_H, sc.offsets(W, H),
                              sc.frame_ids(c.name), bias=bias)[0]


@pytest.mark.parametrize("bias", sc.SHADOW_BIASES)
@pytest.mark.parametrize("k", PLANE_KS)
def test_shadow_across_scale(gpu, k, bias):
    """The mask under the scaled light: shadow_host's at k, and the k = 0 mask (the device's own and
    the host's)."""
    import shadow_cases

    want0 = host_shadow(0, bias)
    sc.assert_shadow_classes(want0)
    shadow_cases.assert_same_mask(device_shadow(0, bias), want0)
    got = device_shadow(k, bias)
    shadow_cases.assert_same_mask(got, host_shadow(k, bias))
    shadow_cases.assert_same_mask(got, want0)


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_rotated_bands_and_block_skip(gpu, name):
    """Three rotated row bands over fake devices: the band record pass's block extents
    (LaunchBlockExtents) and BandMayReach see double-solved and unbounded boxes; every frame the
    oracle's, and the engine's own verification clean."""
    from oracle.srt_oracle import OracleScene
    from simpleraytracer_amd.engine import FrameEngine

    c = sc.case(name)
    F = 6
    inputs = np.random.default_rng(13).random((F, c.h, c.w, 2), dtype=np.float32)
    inputs[0] = sc.offsets(c.w, c.h)
    o = OracleScene(c.path)
    refs = [o.render(c.w, c.h, inputs[f]) for f in range(F)]
    o.close()
    assert same_bits(refs[0], sc.frame(name))  # the guarded frame is among them
    frames = 2 * F
    with FrameEngine(c.path, c.w, c.h, devices=[0] * 3, rows="rotated", queues=2, batch=F) as e:
        e.set_inputs(inputs)
        e.run(2)
        for f in range(frames):
            assert_parity(e.read_frame(f), refs[f % F])
        assert e.verify() == (0, frames)


@pytest.fixture(scope="module")
def order_k0(gpu):
    import simpleraytracer_amd as srt

    scene = srt.DeviceScene(sc.case("k0").path, 0)
    order, _ = scene.spatial_order()
    scene.close()
    order.setflags(write=False)
    return order


@pytest.mark.parametrize("k", ORDER_KS)
def test_spatial_order_across_scale(order_k0, k):
    import simpleraytracer_amd as srt

    c = sc.case(sc.s_name(k))
    scene = srt.DeviceScene(c.path, 0)
    order, _ = scene.spatial_order()
    scene.close()
    assert np.array_equal(order_k0, morton_order_numpy(sc.case("k0").path))
    assert np.array_equal(order, morton_order_numpy(c.path))
    assert np.array_equal(order, order_k0)
