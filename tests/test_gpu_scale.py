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

from types import SimpleNamespace

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


# --- lights, surfaces, materials and moved scenes: what rto*, rtd*, rtv*, rtp* and rtm* compute after the
# hit, on scale_cases' rig and tables. Every comparison is on the uint32 view, a NaN for a NaN
# (shadow_cases.same_bits_or_nan); the host paths equal the numpy restatements on every case
# (test_scale_host.py), so a difference here is the device's.

LIGHT_KS = (-30, -21, 14, 16, 30)   # -30 and +30: nn = N . N subnormal, and +inf
EXACT_KS = (-21, 14, 16)            # nn a normal number everywhere: the bits of the device's own k = 0 answers
SURFACE_KS = (-30, -21, 16, 30)
MOVED = ("k-21", "k16", "k30", "shift_far")
BAND = (37, 5)                      # rows 37..41


class LightRig:
    """S times 2^k on cuda:0 with the lights of sc.rig(k, biased, point), all prepared; every call
    returns numpy arrays."""

    def __init__(self, k, biased=False, point=None):
        import torch

        import simpleraytracer_amd as srt

        self.torch, self.srt, self.k = torch, srt, k
        self.c = sc.case(sc.s_name(k))
        self.stream = torch.cuda.current_stream()
        self.view = srt.DeviceScene(self.c.path, 0)
        self.view.prepare(W, H, self.stream)
        self.specs = sc.rig(k, biased, point)
        self.owned, self.lights = [], []
        for l in self.specs:
            if l.kind == "point":
                light = srt.OmniLight(self.c.path, 0, l.origin)
                light.prepare(l.face_size, self.stream)
                self.lights.append(srt.PointLight(light, l.color, l.falloff, l.bias))
            else:
                light = srt.DeviceScene(self.c.path, 0, camera=l.cam)
                light.prepare(l.wl, l.hl, self.stream)
                self.lights.append(srt.SpotLight(light, l.color, l.falloff, l.bias))
            self.owned.append(light)

    def buffers(self, r0=0, rows=None):
        torch = self.torch
        rows = H - r0 if rows is None else rows
        off = torch.from_numpy(np.array(sc.offsets(W, H)[r0:r0 + rows])).cuda()
        ids = torch.from_numpy(np.array(sc.frame_ids(self.c.name)[r0:r0 + rows])).cuda()
        rgba = torch.full((rows, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        classes = torch.full((len(self.lights), rows, W), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return off, ids, rgba, classes

    def device_surface(self, s):
        up = lambda a: None if a is None else self.torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
        return self.srt.Surface(up(s.normals), up(s.uvs), up(s.texture), s.wrap, s.filter, s.modulate)

    def light(self, r0=0, rows=None, surface=None, material=None):
        """light(), or light_surface() where a surface or a material is given: (rgba, classes)."""
        import litsurface_cases as pc

        off, ids, rgba, classes = self.buffers(r0, rows)
        if surface is None and material is None:
            self.view.light(self.lights, off, ids, rgba, ambient=sc.ambient(), classes=classes, row_begin=r0,
                            row_count=rgba.shape[0], stream=self.stream)
        else:
            self.view.light_surface(self.lights, off, ids, self.device_surface(surface), rgba, ambient=sc.ambient(),
                                    material=pc.host_material(material), classes=classes, row_begin=r0,
                                    row_count=rgba.shape[0], stream=self.stream)
        self.torch.cuda.synchronize()
        return rgba.cpu().numpy(), classes.cpu().numpy()

    def singles(self):
        """(masks (L, H, W), the point light's face plane or None): shadow() / omni_shadow() of every
        light alone at its bias."""
        torch = self.torch
        off, ids, _, _ = self.buffers()
        masks, face_plane = [], None
        for l in self.lights:
            mask = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
            if isinstance(l, self.srt.PointLight):
                face = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
                self.view.omni_shadow(l.light, off, ids, mask, face, bias=l.bias, stream=self.stream)
                torch.cuda.synchronize()
                face_plane = face.cpu().numpy()
            else:
                self.view.shadow(l.scene, off, ids, mask, bias=l.bias, stream=self.stream)
                torch.cuda.synchronize()
            masks.append(mask.cpu().numpy())
        return np.stack(masks), face_plane

    def surface_frame(self, surface):
        torch = self.torch
        off, ids, _, _ = self.buffers()
        planes = {name: torch.full((H, W, ch), float("nan"), dtype=torch.float32, device="cuda")
                  for name, ch in (("normal", 4), ("albedo", 4), ("rgba", 4), ("uv", 2))}
        self.view.surface_frame(off, ids, self.device_surface(surface), stream=self.stream, **planes)
        torch.cuda.synchronize()
        return {name: p.cpu().numpy() for name, p in planes.items()}

    def close(self):
        for o in self.owned:
            o.close()
        self.view.close()


def host_lighting(k, biased=False, surface=None, material=None):
    import lighting_cases
    import litsurface_cases as pc
    from simpleraytracer_amd import device

    c = sc.case(sc.s_name(k))
    lights = lighting_cases.host_lights(sc.rig(k, biased))
    off, ids = sc.offsets(W, H), sc.frame_ids(c.name)
    if surface is None and material is None:
        return device.lighting_host(c.path, W, H, lights, sc.ambient(), off, ids)
    return device.lit_surface_host(c.path, W, H, lights, sc.ambient(), off, ids, surface, pc.host_material(material))


@pytest.fixture(scope="module")
def lit_k0(gpu):
    """The device's own k = 0 answers with and without the point light: light()'s (rgba, classes), and
    light_surface()'s rgba under sc.surface() per shininess. Read-only."""
    out = {}
    for point in (True, False):
        rig = LightRig(0, point=point)
        out[point] = {None: rig.light()}
        for j in sc.SHININESS:
            out[point][j] = rig.light(surface=sc.surface(), material=(sc.SPECULAR, j))
        rig.close()
        for rgba, classes in out[point].values():
            rgba.setflags(write=False)
            classes.setflags(write=False)
    return out


@pytest.mark.parametrize("k", LIGHT_KS)
def test_omni_across_scale(k):
    """omni_shadow's mask and face plane under the point light at the first spot light's eye times
    2^k, at bias 0 and at the bias RIG_BIAS 2^k: omni_shadow_host's at k, and for -21 and 14 the k = 0
    answers. The library refuses an origin beyond 2^16 (DESIGN.md section 2 "Omni shadow"), so k = 14
    stands for the large scales and k = 16, 30 must be refused, on the device as on the host."""
    import omni_cases
    import simpleraytracer_amd as srt
    from simpleraytracer_amd import device

    c = sc.case(sc.s_name(k))
    off, ids = sc.offsets(W, H), sc.frame_ids(c.name)
    if not sc.point_allowed(k):
        with pytest.raises(srt.SrtError, match=r"at most 2\^16 in magnitude"):
            srt.OmniLight(c.path, 0, sc.point_origin(k))
        with pytest.raises(srt.SrtError, match=r"at most 2\^16 in magnitude"):
            device.omni_shadow_host(c.path, W, H, sc.point_origin(k), sc.FACE, off, ids)
        return
    for biased in (False, True):
        rig = LightRig(k, biased)
        masks, face = rig.singles()
        rig.close()
        bias = sc.rig(k, biased)[2].bias
        hmask, hface, _ = device.omni_shadow_host(c.path, W, H, sc.point_origin(k), sc.FACE, off, ids, bias=bias)
        omni_cases.assert_same_mask(masks[2], hmask)
        omni_cases.assert_same_face(face, hface)
        omni_cases.assert_same_mask(masks[2], sc.lit(k, biased).classes[2])
        if k in EXACT_KS and not biased:
            omni_cases.assert_same_mask(masks[2], sc.lit(0).classes[2])
            omni_cases.assert_same_face(face, sc.lit(0).light_facts[2].face)


@pytest.mark.parametrize("k", LIGHT_KS)
def test_lighting_across_scale(monkeypatch, lit_k0, k):
    """scene.light under the rig: the class planes are the single-light calls' and the host's, the RGBA
    the host's and the restatement's -- the whole frame, rows 37..41 as a band, under SRT_CULL_BIN_CAP=8
    and at the bias RIG_BIAS 2^k -- and for EXACT_KS the device's own k = 0 RGBA on the bits. At k = -30
    nn is subnormal on a tenth of the lit pairs; at k = +30 it is +inf on the covering triangles."""
    import lighting_cases
    from shadow_cases import same_bits_or_nan

    want, (hrgba, hclasses) = sc.lit(k), host_lighting(k)
    rig = LightRig(k)
    rgba, classes = rig.light()
    band, band_classes = rig.light(*BAND)
    singles, _ = rig.singles()
    rig.close()
    lighting_cases.assert_same_classes(classes, singles)
    lighting_cases.assert_same_classes(classes, hclasses)
    lighting_cases.assert_same_classes(classes, want.classes)
    same_bits_or_nan("rgba against the host's", rgba, hrgba)
    same_bits_or_nan("rgba against the restatement", rgba, want.rgba)
    rows = slice(BAND[0], BAND[0] + BAND[1])
    same_bits_or_nan("band", band, want.rgba[rows])
    lighting_cases.assert_same_classes(band_classes, want.classes[:, rows])
    if k in EXACT_KS:
        rgba0, classes0 = lit_k0[sc.point_allowed(k)][None]
        lighting_cases.assert_same_classes(classes, classes0)
        same_bits_or_nan("rgba against the device's own k = 0", rgba, rgba0)
    monkeypatch.setenv("SRT_CULL_BIN_CAP", "8")
    rig = LightRig(k)
    capped, capped_classes = rig.light()
    rig.close()
    monkeypatch.delenv("SRT_CULL_BIN_CAP")
    same_bits_or_nan("rgba with overflowed lists", capped, want.rgba)
    lighting_cases.assert_same_classes(capped_classes, want.classes)
    rig = LightRig(k, biased=True)
    rgba, classes = rig.light()
    rig.close()
    hrgba, hclasses = host_lighting(k, biased=True)
    lighting_cases.assert_same_classes(classes, hclasses)
    lighting_cases.assert_same_classes(classes, sc.lit(k, True).classes)
    same_bits_or_nan("biased rgba against the host's", rgba, hrgba)
    same_bits_or_nan("biased rgba against the restatement", rgba, sc.lit(k, True).rgba)


def host_surface(k, s):
    from simpleraytracer_amd import device

    ev = sc.pixel_edges(k)
    got = device.surface_host(sc.case(sc.s_name(k)).path, W, H, ev.pos, ev.ids, s)
    return SimpleNamespace(**dict(zip(("normal", "albedo", "rgba", "uv"), got)))


@pytest.fixture(scope="module")
def surface_k0(gpu):
    """The device's own k = 0 surface planes per (wrap, filter): read-only."""
    import surface_cases as sv

    rig = LightRig(0, point=False)
    out = {(w, f): rig.surface_frame(sc.surface(0, w, f)) for w in sv.WRAPS for f in sv.FILTERS}
    rig.close()
    return out


@pytest.mark.parametrize("k", SURFACE_KS)
def test_surface_across_scale(surface_k0, k):
    """surface_frame with normals, uvs and a texture -- every wrap and filter at k = 16 -- equals the
    restatement at k, surface_host, and (the tables are scale-free) the device's own k = 0 planes."""
    import surface_cases as sv

    modes = [(w, f) for w in sv.WRAPS for f in sv.FILTERS] if k == 16 else [("repeat", "bilinear")]
    rig = LightRig(k, point=False)
    got = {mode: rig.surface_frame(sc.surface(0, *mode)) for mode in modes}
    rig.close()
    for mode in modes:
        sc.check_planes(f"k = {k} {mode} against the restatement", got[mode], sc.surface_planes(k, 0, *mode))
        sc.check_planes(f"k = {k} {mode} against the host", got[mode], host_surface(k, sc.surface(0, *mode)))
        sc.check_planes(f"k = {k} {mode} against k = 0", got[mode],
                        SimpleNamespace(**{n: p.reshape(-1, p.shape[-1]) for n, p in surface_k0[mode].items()}))


@pytest.mark.parametrize("m", sc.SWEEP_MS)
def test_surface_magnitude_sweep(m):
    """The normals table times 2^m at k = 0: Ns . Ns is 0 (m = -75), subnormal (-64), ordinary, huge
    (63) and +inf on more than 100 pixels (64) -- sqrt and the divides at the edges of float32."""
    rig = LightRig(0, point=False)
    got = rig.surface_frame(sc.surface(m))
    rig.close()
    sc.check_planes(f"m = {m} against the restatement", got, sc.surface_planes(0, m))
    sc.check_planes(f"m = {m} against the host", got, host_surface(0, sc.surface(m)))


@pytest.mark.parametrize("k", LIGHT_KS)
def test_lit_surface_across_scale(lit_k0, k):
    """light_surface under the rig, the tables and a material of shininess_log2 0, 1 and 12 (s^4096 is
    subnormal on hundreds of pairs): the restatement's and the host's RGBA, and for EXACT_KS the device's
    own k = 0 RGBA."""
    import lighting_cases
    from shadow_cases import same_bits_or_nan

    rig = LightRig(k)
    got = {j: rig.light(surface=sc.surface(), material=(sc.SPECULAR, j)) for j in sc.SHININESS}
    alone, _ = rig.light(surface=sc.black_surface(), material=(sc.SPECULAR, 12))
    rig.close()
    # under a black texture the pixel is specular . S alone: the subnormal highlights are the output
    same_bits_or_nan("the highlight alone", alone, sc.lit_surface(k, 0, (sc.SPECULAR, 12), black=True))
    same_bits_or_nan("the highlight alone, against the host's", alone,
                     host_lighting(k, surface=sc.black_surface(), material=(sc.SPECULAR, 12))[0])
    for j, (rgba, classes) in got.items():
        material = (sc.SPECULAR, j)
        lighting_cases.assert_same_classes(classes, sc.lit(k).classes)
        same_bits_or_nan(f"shininess_log2 = {j}: rgba", rgba, sc.lit_surface(k, 0, material))
        same_bits_or_nan(f"shininess_log2 = {j}: rgba against the host's", rgba,
                         host_lighting(k, surface=sc.surface(), material=material)[0])
        if k in EXACT_KS:
            same_bits_or_nan(f"shininess_log2 = {j}: rgba against the device's own k = 0", rgba,
                             lit_k0[sc.point_allowed(k)][j][0])


@pytest.mark.parametrize("m", (sc.SWEEP_MS[0], sc.SWEEP_MS[-1]))
def test_lit_surface_under_a_degenerate_table(m):
    """Ns . Ns = 0 (u is +-inf or NaN) and +inf (u = 0): every such u clamps to a zero or unit cosine, so
    the lit frame holds no NaN; the restatement's and the host's bits."""
    from shadow_cases import same_bits_or_nan

    material = (sc.SPECULAR, 12)
    rig = LightRig(0)
    rgba, _ = rig.light(surface=sc.surface(m), material=material)
    rig.close()
    assert not np.isnan(rgba).any()
    same_bits_or_nan(f"m = {m}", rgba, sc.lit_surface(0, m, material))
    same_bits_or_nan(f"m = {m} against the host's", rgba, host_lighting(0, surface=sc.surface(m), material=material)[0])


@pytest.mark.parametrize("reorder", [True, False], ids=["reorder", "keep_order"])
@pytest.mark.parametrize("name", MOVED)
def test_moved_scene_across_scale(name, reorder):
    """A scene made from the k = 0 file and moved -- set_vertices, then set_camera -- to S times 2^k or
    to the far translation answers as a fresh scene there: the oracle's frame through the cull and bvh
    traces, the restated spatial order (reorder=True), the host's shadow mask under a light moved the same
    way; moved back, the first k = 0 frame bit for bit."""
    import shadow_cases
    import torch

    import simpleraytracer_amd as srt
    from scenefile import read_scene
    from simpleraytracer_amd import device

    c0, c = sc.case("k0"), sc.case(name)
    cam0, _, v0, _ = read_scene(c0.path)
    cam, _, v, _ = read_scene(c.path)
    shift = sc.SHIFTS.get(name)
    light_cam = sc.light_camera(c.k) if c.k is not None else \
        (*[float(x) for e in sc.scaled_camera(sc.LIGHT_EYE, sc.LIGHT_LOOK, 0, shift) for x in e], *sc.LIGHT_UP, sc.LIGHT_VFOV)
    stream = torch.cuda.current_stream()
    up = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    off, ids = up(sc.offsets(W, H)), up(sc.frame_ids(name))
    view, light = srt.DeviceScene(c0.path, 0), srt.DeviceScene(c0.path, 0, camera=sc.light_camera(0))
    view.prepare(W, H, stream)
    light.prepare(sc.LIGHT_W, sc.LIGHT_H, stream)

    def trace(variant):
        out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        view.trace(off, out, variant=variant, stream=stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    first = {variant: trace(variant) for variant in ("cull", "bvh")}
    moved_v = up(v)
    for scene, camera in ((view, cam), (light, light_cam)):
        scene.set_vertices(moved_v, reorder=reorder, stream=stream)
        scene.set_camera(camera, reorder=reorder, stream=stream)
    moved = {variant: trace(variant) for variant in ("cull", "bvh")}
    order, _ = view.spatial_order()
    mask = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
    view.shadow(light, off, ids, mask, None, bias=0.0, stream=stream)
    torch.cuda.synchronize()
    mask = mask.cpu().numpy()
    home_v = up(v0)
    view.set_vertices(home_v, reorder=reorder, stream=stream)
    view.set_camera(cam0, reorder=reorder, stream=stream)
    back = {variant: trace(variant) for variant in ("cull", "bvh")}
    home_order, _ = view.spatial_order()
    view.close()
    light.close()
    for variant in ("cull", "bvh"):
        assert_parity(first[variant], sc.frame("k0"))
        assert_parity(moved[variant], sc.frame(name))
        assert same_bits(back[variant], first[variant]), f"{variant}: moved back, the frame is not the first one"
    if reorder:
        assert np.array_equal(order, morton_order_numpy(c.path))
        assert np.array_equal(home_order, morton_order_numpy(c0.path))
    want = device.shadow_host(c.path, W, H, light_cam, sc.LIGHT_W, sc.LIGHT_H, sc.offsets(W, H), sc.frame_ids(name),
                              bias=0.0)[0]
    shadow_cases.assert_same_mask(mask, want)
    if c.k is not None:
        shadow_cases.assert_same_mask(mask, host_shadow(c.k, 0.0))
