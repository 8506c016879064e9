"""Sampled visibility on the host (include/srt_visibility.h: rtaRaysHost, rtaVisibilityHost), no GPU.

H1: the host's rays equal a numpy float32 restatement of DESIGN.md section 2 "Visibility", bit for bit.
H2: the host's count equals the count over rtrOccludedHost of the host's rays.
H3: the identity rotation gives the bytes of no rotation table.
H4: every refusal names its field.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import visibility_cases as vc
from simpleraytracer_amd import _native, device
from simpleraytracer_amd import samples as sm

f32 = np.float32
W, H = vc.FRAMES[0]


def _generators(samples=5):
    return {
        "hemisphere": vc.hemisphere(samples, 0.3),
        "hemisphere_rotated": vc.hemisphere(samples, 0.3, True),
        "area": vc.area_light(samples),
        "mirror": vc.mirror(),
    }


@pytest.mark.parametrize("kind", ["hemisphere", "hemisphere_rotated", "area", "mirror"])
@pytest.mark.parametrize("name", ["q", "cornell", "soup"])
def test_host_rays_equal_the_numpy_restatement(name, kind):
    """H1: 600 positions with their hit ids, then ids -1, n, a sentinel, scene Q's point and collinear
    triangles (step 3) and 40 ids that do not hit where they are asked; points-call rotation indices."""
    c = vc.points_case(name, W, H)
    gen = _generators()[kind]
    got = device.rays_host(c.path, W, H, c.pos, c.ids, gen)
    assert got.shape == (gen.count, len(c.ids), 8) and got.dtype == f32
    want = vc.restate_rays(c.path, W, H, c.pos, c.ids, gen)
    vc.same_bits(f"{name} {kind} rays", got, want)
    live = (got[0, :, 4:7] != 0).any(axis=1)
    assert live[:600].sum() >= 100, "too few elements on a surface to compare"
    assert not live[600:604].any(), "ids outside the scene give zero rays"
    assert (got[:, ~live] == 0).all()
    if name == "q":
        assert not live[604:606].any(), "the point and the collinear triangle have no normal: zero rays"
    assert live[-40:].any(), "no id that misses its position produced rays"


def test_frame_rotation_indices_in_the_restatement():
    """The restatement under a frame call's rotation indices equals the host asked index by index
    (what the GPU tests compare a frame call against)."""
    w, h = vc.FRAMES[1]
    _, pos, ids = vc.frame_elements("cornell", w, h, True)
    gen = vc.hemisphere(3, 1.0, True)
    turns = vc.frame_turns(w, h)
    vc.same_bits("rays", vc.host_rays(vc.scene_path("cornell"), w, h, pos, ids, gen, turns),
                 vc.restate_rays(vc.scene_path("cornell"), w, h, pos, ids, gen, turns))


@pytest.mark.parametrize("samples", [1, 7, 8, 64])
@pytest.mark.parametrize("mix", ["cornell_hemisphere", "soup_area"])
def test_host_visibility_is_the_count_over_the_rays(mix, samples):
    """H2: visible = the number of the S rays rtrOccludedHost leaves at 0; fraction = visible / S."""
    name, make = vc.MIXES[mix]
    path = vc.scene_path(name)
    _, pos, ids = vc.frame_elements(name, W, H, True)
    if samples == 64:  # (a quarter of the frame keeps the brute-force host inside a few seconds)
        pos, ids = pos[::4], ids[::4]
    gen = make(samples, True if mix == "cornell_hemisphere" else None)
    visible, fraction = device.visibility_host(path, W, H, pos, ids, gen)
    assert visible.dtype == np.uint8 and fraction.dtype == f32
    rays = device.rays_host(path, W, H, pos, ids, gen)
    occ = device.occluded_host(path, rays.reshape(-1, 8)).reshape(samples, len(ids))
    want = (occ == 0).sum(axis=0).astype(np.uint8)
    assert np.array_equal(visible, want)
    vc.same_bits("fraction", fraction, vc.fraction_of(want, samples))
    off = (ids < 0)
    assert off.any() or name == "cornell"
    assert (visible[off] == samples).all(), "an element off a surface sees every ray"
    if samples == 8:
        vc.assert_mix(visible, ids, device.scene_triangles(path), samples)


@pytest.mark.parametrize("mix", list(vc.MIXES))
def test_the_mixes_hold(mix):
    """The three inputs of the GPU tests meet the mix condition on the host answer (48 x 32, S = 8)."""
    name, _ = vc.MIXES[mix]
    _, _, ids = vc.frame_elements(name, W, H, False)
    _, visible, fraction = vc.mix_answer(mix, W, H, False)
    vc.assert_mix(visible, ids, device.scene_triangles(vc.scene_path(name)), 8)
    vc.same_bits("fraction", fraction, vc.fraction_of(visible, 8))


def test_the_range_keeps_a_ray_off_its_own_surface():
    """Cornell, hemisphere, tmax = 0.5: with tmin = 0 many surface pixels are fully occluded by their
    own triangle; with tmin = 2^-10 none are (the figure in include/srt_visibility.h)."""
    path = vc.scene_path("cornell")
    _, pos, ids = vc.frame_elements("cornell", W, H, False)
    surface = ids >= 0
    zero, _ = device.visibility_host(path, W, H, pos, ids, vc.hemisphere(8, 0.5, tmin=0.0))
    lifted, _ = device.visibility_host(path, W, H, pos, ids, vc.hemisphere(8, 0.5))
    assert (zero[surface] == 0).sum() >= 0.2 * surface.sum()
    assert (lifted[surface] == 0).sum() == 0


def test_identity_rotation_is_no_rotation():
    """H3: (1, 0) x 16 gives the bytes of no table."""
    c = vc.points_case("soup", W, H)
    plain = vc.hemisphere(8, 0.3)
    turned = device.Hemisphere(plain.samples, plain.tmin, plain.tmax, np.tile(f32([1, 0]), (16, 1)))
    vc.same_bits("rays", device.rays_host(c.path, W, H, c.pos, c.ids, turned),
                 device.rays_host(c.path, W, H, c.pos, c.ids, plain))
    a, b = device.visibility_host(c.path, W, H, c.pos, c.ids, turned), device.visibility_host(c.path, W, H, c.pos, c.ids, plain)
    assert np.array_equal(a[0], b[0])
    vc.same_bits("fraction", a[1], b[1])


def test_sample_tables():
    for s in (1, 7, 8, 16, 64):
        d = sm.cosine_hemisphere(s, 5)
        assert d.shape == (s, 3) and d.dtype == f32 and (d[:, 2] > 0).all()
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
        assert np.array_equal(d, sm.cosine_hemisphere(s, 5)) and not np.array_equal(d, sm.cosine_hemisphere(s, 6))
        ab = sm.area_samples(s, 5)
        assert ab.shape == (s, 2) and ab.dtype == f32 and (ab >= 0).all() and (ab < 1).all()
        g = sm.grid_side(s)
        cells = np.floor(ab.astype(np.float64) * g).astype(int)
        assert np.array_equal(cells, np.stack([np.arange(s) % g, np.arange(s) // g], 1)), "one sample per grid cell"
    # cosine-weighted: the mean of lz over many samples is 2 / 3
    assert abs(float(sm.cosine_hemisphere(64, 1)[:, 2].mean()) - 2 / 3) < 0.03
    r = sm.rotations(4)
    assert r.shape == (16, 2) and r.dtype == f32
    assert np.abs((r.astype(np.float64) ** 2).sum(axis=1) - 1).max() <= 2.0 ** -22


def _gen(kind=_native.RTA_HEMISPHERE, samples=4, table=None, size=None, corner=(0, 0, 0), eu=(1, 0, 0), ev=(0, 1, 0)):
    table = np.zeros((64, 3), f32) if table is None else table
    c3 = ctypes.c_float * 3
    return _native.RtaGenerator(ctypes.sizeof(_native.RtaGenerator) if size is None else size, kind, samples,
                                0 if table is False else table.ctypes.data, 0, c3(*corner), c3(*eu), c3(*ev), 0.0, 1.0), table


def test_refusals_name_their_field():
    """H4: every refusal of include/srt_visibility.h, through the host forms (the device forms share the checks)."""
    L = _native.lib()
    path = vc.scene_path("cornell").encode()
    pos, ids = np.full((1, 2), 0.5, f32), np.zeros(1, np.int32)
    vis, frac, rays = np.zeros(1, np.uint8), np.zeros(1, f32), np.zeros((64, 1, 8), f32)
    out = _native.RtaOutputs(ctypes.sizeof(_native.RtaOutputs), vis.ctypes.data, frac.ctypes.data)

    def visibility(g, o=out):
        return L.rtaVisibilityHost(path, W, H, pos.ctypes.data, ids.ctypes.data, 1, ctypes.byref(g), ctypes.byref(o))

    def generate(g):
        return L.rtaRaysHost(path, W, H, pos.ctypes.data, ids.ctypes.data, 1, ctypes.byref(g), rays.ctypes.data)

    def refused(call, g, text):
        assert call(g) == -1
        assert text in _native.last_error(), _native.last_error()

    good, keep = _gen()
    assert visibility(good) == 0 and generate(good) == 0
    for call in (visibility, generate):
        refused(call, _gen(size=8)[0], "rta_generator.struct_size")
        refused(call, _gen(samples=0)[0], "rta_generator.samples")
        refused(call, _gen(samples=65)[0], "rta_generator.samples")
        refused(call, _gen(table=False)[0], "rta_generator.d_samples")
        refused(call, _gen(kind=7)[0], "rta_generator.kind")
        for field in ("corner", "eu", "ev"):
            for bad in (np.nan, np.inf, -np.inf):
                refused(call, _gen(_native.RTA_AREA, **{field: (0.0, bad, 1.0)})[0], f"rta_generator.{field}")
    refused(visibility, _gen(_native.RTA_MIRROR, samples=1)[0], "RTA_MIRROR")
    refused(generate, _gen(_native.RTA_MIRROR, samples=2)[0], "rta_generator.samples")
    assert generate(_gen(_native.RTA_MIRROR, samples=1, table=False)[0]) == 0  # (a mirror has no table)
    bad_out = _native.RtaOutputs(4, vis.ctypes.data, frac.ctypes.data)
    assert visibility(good, bad_out) == -1 and "rta_outputs.struct_size" in _native.last_error()
    # the device forms: the same checks after the handle's
    assert L.rtaVisibilityPointsAsync(None, None, None, 0, ctypes.byref(good), ctypes.byref(out), None) == -1
    assert _native.last_error() == "Bad scene handle"
    assert L.rtaVisibilityFrameAsync(None, None, None, 0, 0, ctypes.byref(good), ctypes.byref(out), None) == -1
    assert L.rtaRaysPointsAsync(None, None, None, 0, ctypes.byref(good), None, None) == -1
    assert L.rtaRaysFrameAsync(None, None, None, 0, 0, ctypes.byref(good), None, None) == -1
    # a NULL plane is not written; no plane at all reads nothing
    vis[:], frac[:] = 77, -5.0
    only = _native.RtaOutputs(ctypes.sizeof(_native.RtaOutputs), vis.ctypes.data, 0)
    assert visibility(good, only) == 0 and vis[0] <= 4 and frac[0] == -5.0
    none = _native.RtaOutputs(ctypes.sizeof(_native.RtaOutputs), 0, 0)
    assert L.rtaVisibilityHost(path, W, H, None, None, 1, ctypes.byref(good), ctypes.byref(none)) == 0
    assert L.rtaRaysHost(path, W, H, None, None, 0, ctypes.byref(good), None) == 0
    del keep
    with pytest.raises(ValueError, match=r"samples must be \(S, 3\)"):
        device.Hemisphere(np.zeros((4, 2), f32), 0.0, 1.0)
    with pytest.raises(ValueError, match=r"rotations must be \(16, 2\)"):
        device.Hemisphere(np.zeros((4, 3), f32), 0.0, 1.0, np.zeros((4, 2), f32))
