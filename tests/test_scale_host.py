"""Coordinate range on the host: the CPU backend and the host restatements (query_host, layers_host,
attributes_host, shadow_host) on tests/scale_cases.py's scenes -- scene S times 2^k across the float
solve's range, translated far from the origin, under a 1 degree view, and the cloud under telephoto,
fisheye, strip-frame and rolled cameras -- against the oracle, on the bits. No GPU.

They share csrc/screen_box.h and the exactness argument with the device path, so a frame that differs
here is a flaw in the definition or in the cull's constants, one that differs only on the device is
a device bug (test_gpu_scale.py). The case guards (scale_cases) run with the oracle's answers.

The second half puts what the light, surface and material families compute after the hit through the
same scales and through float32's edges (scale_cases' rig, tables and magnitude sweep): lighting_host,
omni_shadow_host, surface_host and lit_surface_host against the numpy restatements, a NaN for a NaN,
with the guards that keep those cases, and the device tests that share them, from passing vacuously.
"""
from __future__ import annotations

import numpy as np
import pytest

import layers_cases as lc
import query_cases as qc
import scale_cases as sc
import simpleraytracer_amd as srt
import simpleraytracer_amd.device as device

ATTR_KS = (-21, 16)
SHADOW_KS = (-21, 16, 30)


@pytest.fixture
def cpu(monkeypatch):
    monkeypatch.setenv("ML_VISIBLE_DEVICES", "cpu")
    monkeypatch.setenv("SRT_CPU_THREADS", "4")


def assert_frame_bits(got, want, what):
    bad = np.argwhere(sc.bits(got) != sc.bits(want))
    assert bad.size == 0, (f"{what}: {len(bad)} values differ, first at (y, x, c) = {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("name", [sc.s_name(k) for k in sc.HOST_KS] + list(sc.EXTRA_NAMES) + list(sc.CLOUD_NAMES))
def test_cpu_backend_equals_oracle(cpu, name):
    c = sc.case(name)
    for kind in ("rnd", "half"):
        want = sc.frame(name, kind)
        with np.errstate(all="ignore"):
            got = srt.render(c.path, c.w, c.h, sc.offsets(c.w, c.h) if kind == "rnd" else None)
        assert_frame_bits(got, want, f"{name}, {kind} offsets")


@pytest.mark.parametrize("k", sc.HOST_KS)
def test_query_and_layers_host_across_scale(k):
    """Exact against the oracle at every k; the oracle's own answers are those of k = 0 with t times
    2^k (asserted in scale_cases.answers), so the host's are too."""
    c = sc.case(sc.s_name(k))
    pos, want_ids, want_t = sc.answers(c.name)
    ids, t = device.query_host(c.path, c.w, c.h, pos)
    qc.assert_same(ids, t, want_ids, want_t)
    _, l_ids, l_t = sc.layers(c.name)
    ids4, t4 = device.layers_host(c.path, c.w, c.h, pos, sc.LAYERS)
    lc.assert_same(ids4, t4, l_ids, l_t)
    _, ids0, t0 = sc.answers(sc.s_name(0))
    _, l_ids0, l_t0 = sc.layers(sc.s_name(0))
    assert np.array_equal(ids, ids0) and np.array_equal(ids4, l_ids0)
    qc.assert_same(ids, t, ids0, sc.scaled_t(t0, k))
    lc.assert_same(ids4, t4, l_ids0, sc.scaled_t(l_t0, k))


@pytest.mark.parametrize("name", [sc.s_name(k) for k in sc.HOST_KS] + list(sc.EXTRA_NAMES) + list(sc.CLOUD_NAMES))
def test_screen_boxes_contain_the_exact_region(name):
    """The cull's exactness argument on the cases' own records: the box of the solve the record pass
    takes, and the double solve's, contain the exact (rational) corners of the slack-shifted region
    of every enabled record -- test_screen_box's check, on coefficients from 2^-67 to 2^67 and on
    the telephoto and fisheye records. The share the float solve answers is float_share's."""
    import test_screen_box as tsb

    recs = sc.enabled_records(name)
    fast = sum(bool(tsb.check([np.float32(v) for v in rec])) for rec in recs)
    assert fast == round(sc.float_share(name) * len(recs))
    if sc.case(name).k is not None:
        sc.assert_float_share(sc.case(name).k)


def attributes(name):
    c = sc.case(name)
    pos, ids, _ = sc.answers(name)
    return device.attributes_host(c.path, c.w, c.h, pos, ids)


@pytest.mark.parametrize("k", ATTR_KS)
def test_attributes_host_across_scale(k):
    """Depth scales by 2^k; barycentrics, normal and albedo are those of k = 0: bit for bit."""
    _, ids, t = sc.answers(sc.s_name(k))
    depth0, bary0, normal0, albedo0 = attributes(sc.s_name(0))
    depth, bary, normal, albedo = attributes(sc.s_name(k))
    assert (ids >= 0).sum() >= 500
    lc.same_bits("depth vs the oracle's t", depth, t)
    lc.same_bits("depth", depth, sc.scaled_t(depth0, k))
    lc.same_bits("bary", bary, bary0)
    lc.same_bits("normal", normal, normal0)
    lc.same_bits("albedo", albedo, albedo0)


def shadow_mask(k, bias):
    c = sc.case(sc.s_name(k))
    mask, _ = device.shadow_host(c.path, c.w, c.h, sc.light_camera(k), sc.LIGHT_W, sc.LIGHT_H, sc.offsets(c.w, c.h),
                                 sc.frame_ids(c.name), bias=bias)
    return mask


@pytest.mark.parametrize("bias", sc.SHADOW_BIASES)
def test_shadow_host_across_scale(bias):
    """The light's camera scales with the scene and the bias is relative: the mask is that of k = 0."""
    want = shadow_mask(0, bias)
    sc.assert_shadow_classes(want)
    for k in SHADOW_KS:
        got = shadow_mask(k, bias)
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, f"k = {k}: {bad.size} classes differ from k = 0, first at pixel {bad[0]}"


# --- lights, surfaces and materials: the host paths against the numpy restatements (scale_cases) ---

W_, H_ = sc.W, sc.H
EXACT_KS = (-21, 14, 16)  # nn stays a normal number: the answers are those of k = 0 on the bits
SWEEP_LO, SWEEP_SUB, _, SWEEP_BIG, SWEEP_HI = sc.SWEEP_MS


def test_rig_guards():
    """Conditions on the inputs (scale_cases records the counts): no new test passes vacuously."""
    from shadow_cases import LIT, SHADOWED

    l0 = sc.lit(0)
    hit = l0.fa.surface
    for j, plane in enumerate(l0.classes):
        shadowed, lit_count = int((plane == SHADOWED).sum()), int((plane == LIT).sum())
        print(f"k = 0, light {j}: {shadowed} shadowed, {lit_count} lit, {int(l0.terms[j].contributes.sum())} contributing")
        assert shadowed >= 100 and lit_count >= 100
    several = sum(t.contributes.astype(int) for t in l0.terms) >= 2
    print(f"k = 0: {int(hit.sum())} hit pixels, {int(several.sum())} under two or more lights")
    assert several.sum() >= hit.sum() / 5
    lo = sc.lit(-30)
    pairs = np.stack([t.contributes for t in lo.terms])
    nn = np.broadcast_to(lo.fa.nn, pairs.shape)
    sub, zero = int((sc.subnormal(nn) & pairs).sum()), int(((nn == 0) & pairs).sum())
    print(f"k = -30: {int(pairs.sum())} (lit pixel, light) pairs, nn subnormal in {sub}, nn == 0 in {zero}")
    assert sub >= 0.05 * pairs.sum()
    hi = sc.lit(30)
    inf = int((np.isinf(hi.fa.nn) & hi.fa.surface).sum())
    print(f"k = +30: nn == +inf at {inf} pixels")
    assert inf >= 100 and (hi.fa.nn[hi.fa.surface] > 0).all()
    assert [sc.point_allowed(k) for k in sc.RIG_KS] == [True, True, True, True, False, False]


def test_sweep_and_shininess_guards():
    counts = {}
    for m in sc.SWEEP_MS:
        nn = sc.table_nn(m)
        counts[m] = (len(nn), int(sc.subnormal(nn).sum()), int((nn == 0).sum()), int(np.isinf(nn).sum()))
        print(f"normals table times 2^{m}: {counts[m][0]} hit pixels, Ns.Ns subnormal at {counts[m][1]}, 0 at "
              f"{counts[m][2]}, +inf at {counts[m][3]}")
    assert counts[SWEEP_SUB][1] >= 0.05 * counts[SWEEP_SUB][0]
    assert counts[SWEEP_LO][2] >= 100 and counts[SWEEP_HI][3] >= 100
    assert counts[SWEEP_BIG][3] == 0 and counts[0][1:] == (0, 0, 0)
    pairs = sum(int((sc.subnormal(s) & on).sum()) for s, on in sc.highlights(0, 12))
    print(f"shininess_log2 = 12: the squared-out s is subnormal in {pairs} (pixel, light) pairs")
    assert pairs >= 16
    # ... and they reach the output where the albedo plane is black: rgb = specular . S alone
    alone = sc.lit_surface(0, 0, (sc.SPECULAR, 12), black=True)[..., :3]
    visible = int(sc.subnormal(alone).any(axis=-1).sum())
    print(f"shininess_log2 = 12 under the black texture: {visible} pixels with a subnormal rgb value")
    assert visible >= 16


def host_rig(k, biased=False, point=None):
    import lighting_cases

    return lighting_cases.host_lights(sc.rig(k, biased, point))


@pytest.mark.parametrize("k", sc.RIG_KS)
def test_lighting_and_omni_host_across_scale(k):
    """lighting_host and omni_shadow_host equal the restatement at every k, at bias 0 and at the bias
    RIG_BIAS 2^k; while nn is a normal number the bias-0 answers are those of k = 0 on the bits."""
    import lighting_cases
    import omni_cases
    from shadow_cases import same_bits_or_nan

    c = sc.case(sc.s_name(k))
    off, ids = sc.offsets(W_, H_), sc.frame_ids(c.name)
    for biased in (False, True):
        want = sc.lit(k, biased)
        rgba, classes = device.lighting_host(c.path, W_, H_, host_rig(k, biased), sc.ambient(), off, ids)
        lighting_cases.assert_same_classes(classes, want.classes)
        same_bits_or_nan(f"k = {k}, biased = {biased}: rgba", rgba, want.rgba)
        if sc.point_allowed(k):
            light = sc.rig(k, biased)[2]
            mask, face, _ = device.omni_shadow_host(c.path, W_, H_, light.origin, sc.FACE, off, ids, bias=light.bias)
            omni_cases.assert_same_mask(mask, want.classes[2])
            omni_cases.assert_same_face(face, want.light_facts[2].face)
    if k in EXACT_KS:
        want0 = sc.lit(0, point=sc.point_allowed(k))
        lighting_cases.assert_same_classes(sc.lit(k).classes, want0.classes)
        same_bits_or_nan(f"k = {k}: rgba against k = 0", sc.lit(k).rgba, want0.rgba)
    if not sc.point_allowed(k):
        with pytest.raises(device.SrtError, match="at most 2\\^16 in magnitude"):
            device.omni_shadow_host(c.path, W_, H_, sc.point_origin(k), sc.FACE, off, ids)


def host_surface_planes(k, s):
    c = sc.case(sc.s_name(k))
    ev = sc.pixel_edges(k)
    return dict(zip(("normal", "albedo", "rgba", "uv"), device.surface_host(c.path, W_, H_, ev.pos, ev.ids, s)))


@pytest.mark.parametrize("k", sc.RIG_KS)
def test_surface_host_across_scale(k):
    """surface_host equals the restatement at every k -- every wrap and filter at k = 16 -- and, the
    tables being scale-free, the planes of k = 0 on the bits."""
    import surface_cases as sv

    modes = [(w, f) for w in sv.WRAPS for f in sv.FILTERS] if k == 16 else [("repeat", "bilinear")]
    for wrap, filt in modes:
        got = host_surface_planes(k, sc.surface(0, wrap, filt))
        sc.check_planes(f"k = {k} {wrap} {filt}", got, sc.surface_planes(k, 0, wrap, filt))
        sc.check_planes(f"k = {k} {wrap} {filt} against k = 0", got, sc.surface_planes(0, 0, wrap, filt))


@pytest.mark.parametrize("m", sc.SWEEP_MS)
def test_surface_host_magnitude_sweep(m):
    """The normals table times 2^m at k = 0: Ns . Ns 0, subnormal, ordinary, huge and +inf."""
    sc.check_planes(f"m = {m}", host_surface_planes(0, sc.surface(m)), sc.surface_planes(0, m))


@pytest.mark.parametrize("k", sc.RIG_KS)
def test_lit_surface_host_across_scale(k):
    import lighting_cases
    import litsurface_cases as pc
    from shadow_cases import same_bits_or_nan

    c = sc.case(sc.s_name(k))
    off, ids = sc.offsets(W_, H_), sc.frame_ids(c.name)
    for material in [None] + [(sc.SPECULAR, j) for j in sc.SHININESS]:
        rgba, classes = device.lit_surface_host(c.path, W_, H_, host_rig(k), sc.ambient(), off, ids, sc.surface(),
                                                pc.host_material(material))
        lighting_cases.assert_same_classes(classes, sc.lit(k).classes)
        want = sc.lit_surface(k, 0, material)
        same_bits_or_nan(f"k = {k}, material {material}", rgba, want)
        if k in EXACT_KS:
            same_bits_or_nan(f"k = {k}, material {material}: against k = 0", rgba,
                             sc.lit_surface(0, 0, material, point=sc.point_allowed(k)))
    material = (sc.SPECULAR, 12)  # the highlight alone: its subnormal values are the pixel
    rgba, _ = device.lit_surface_host(c.path, W_, H_, host_rig(k), sc.ambient(), off, ids, sc.black_surface(),
                                      pc.host_material(material))
    same_bits_or_nan(f"k = {k}, the highlight alone", rgba, sc.lit_surface(k, 0, material, black=True))


@pytest.mark.parametrize("m", (SWEEP_LO, SWEEP_HI))
def test_lit_surface_host_under_a_degenerate_table(m):
    """Ns . Ns = 0 or +inf: u is NaN (0 / 0, inf / inf) or 0; a NaN u clamps to a zero contribution, so
    the lit frame holds no NaN."""
    import litsurface_cases as pc
    from shadow_cases import same_bits_or_nan

    c = sc.case("k0")
    material = (sc.SPECULAR, 12)
    rgba, _ = device.lit_surface_host(c.path, W_, H_, host_rig(0), sc.ambient(), sc.offsets(W_, H_), sc.frame_ids("k0"),
                                      sc.surface(m), pc.host_material(material))
    u = sc.surface_planes(0, m).normal[:, :3]
    assert (~np.isfinite(u)).any(axis=1).sum() >= 100 if m == SWEEP_LO else ((u == 0).all(axis=1).sum() >= 100)
    assert not np.isnan(rgba).any()
    same_bits_or_nan(f"m = {m}", rgba, sc.lit_surface(0, m, material))


def test_scene_q_is_unchanged_and_s_shares_its_geometry(tmp_path):
    """Scene S's vertices at k = 0 are scene Q's file's, its camera is the dyadic one."""
    from scenefile import read_scene

    _, _, vq, _ = read_scene(qc.write_scene_q(tmp_path / "q.srt"))
    cam, bg, vs, alb = read_scene(sc.case(sc.s_name(0)).path)
    assert np.array_equal(vq.view(np.uint32), vs.view(np.uint32))
    assert np.array_equal(cam, np.float32([*sc.S_EYE, *sc.S_LOOK, *sc.S_UP, sc.S_VFOV]))
    assert alb.min() >= 0.2 and alb.max() <= 1.0 and np.array_equal(bg, np.float32(sc.BACKGROUND))
    _, _, v16, _ = read_scene(sc.case(sc.s_name(16)).path)
    assert np.array_equal(v16, vs * np.float32(65536.0))
