"""Shared cases of the direct-lighting tests (test_lighting_host.py, test_gpu_lighting.py): the
lights, the numpy float32 restatement of DESIGN.md section 2 "Lighting" and the expected class planes
and RGBA -- from the oracle and numpy, never from the library. Not a test module.

Expected values: a light's class plane is shadow_cases.restate (a spot light: the view's file and a
file of the same triangles under the light's camera) or omni_cases' facts and mask_of (a point
light); N is the cross product of the scene file's vertices in float32 (e1 x e2, each component two
products and a difference); t is oracle.closest_hit on the pixel's own record; the accumulation is
the definition in numpy float32 arrays, one rounding per operation. All frames are 160 x 96. A
view's facts and a light's class plane are computed once per session and shared read-only.
"""
from __future__ import annotations

import functools
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import omni_cases as oc
import shadow_cases as sc
from oracle import srt_oracle as oracle

f32 = np.float32
W, H = sc.W, sc.H
BACKGROUND = (0.1, 0.2, 0.3)  # shadow_cases.write_with_camera's
BELOW_CAM = (0.0, -4.0, 4.0, 0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 60.0)  # under scene T's floor, looking up
SPOT_IN = (2.0, 2.6, 2.0, -0.5, -1.0, 4.5, 0.0, 1.0, 0.0, 70.0)   # inside the room
SPOT_IN2 = (-2.0, 2.5, 5.5, 0.5, -1.0, 3.0, 0.0, 1.0, 0.0, 70.0)
ORIGIN2 = (-1.5, 2.0, 2.5)  # the second point light of "full"
AMBIENT = (0.05, 0.04, 0.03)


def spot(cam, wl, hl, color, falloff=0.0, bias=0.0):
    return SimpleNamespace(kind="spot", cam=tuple(float(v) for v in cam), wl=wl, hl=hl, color=color, falloff=falloff,
                           bias=bias)


def point(origin, face_size, color, falloff=0.0, bias=0.0):
    return SimpleNamespace(kind="point", origin=tuple(float(v) for v in origin), face_size=face_size, color=color,
                           falloff=falloff, bias=bias)


def headlight(cam, color=(1.0, 1.0, 1.0)):
    return spot(cam, W, H, color)


# name -> (scene, view, lights); scene "T": shadow_cases' scene T under VIEW_CAM, "room": omni_cases' room
def _t4():
    b = sc.BIASES
    return [spot(sc.LIGHT_CAM, sc.WL, sc.HL, (1.0, 0.9, 0.8), 0.0, b[0]),
            spot(sc.VIEW_CAM, W, H, (0.2, 0.3, 0.9), 0.0, b[1]),
            spot(sc.AWAY_CAM, sc.WL, sc.HL, (0.5, 0.5, 0.5), 0.0, b[0]),
            spot(BELOW_CAM, sc.WL, sc.HL, (0.9, 0.2, 0.1), 9.0, b[1])]


def _room(view, face_size=64):
    return [point(oc.ORIGIN, face_size, (1.0, 0.8, 0.6), 4.0, oc.BIASES[1]),
            spot(SPOT_IN, sc.WL, sc.HL, (0.3, 0.6, 1.0), 0.0, oc.BIASES[0]),
            headlight(oc.VIEWS[view], (0.25, 0.25, 0.25))]


def _full():
    return [point(oc.ORIGIN, 64, (1.0, 0.8, 0.6), 4.0, oc.BIASES[1]),
            spot(SPOT_IN, sc.WL, sc.HL, (0.3, 0.6, 1.0), 0.0, oc.BIASES[0]),
            point(ORIGIN2, 64, (0.2, 0.9, 0.3), 2.5, oc.BIASES[0]),
            headlight(oc.VIEWS["A"], (0.25, 0.25, 0.25)),
            spot(oc.VIEWS["B"], W, H, (0.7, 0.1, 0.7), 6.0, oc.BIASES[1]),
            spot(SPOT_IN2, sc.WL, sc.HL, (0.1, 0.1, 0.6), 0.0, oc.BIASES[0])]


CASES = {
    "T4": ("T", None, _t4),
    "roomA": ("room", "A", functools.partial(_room, "A")),
    "roomB": ("room", "B", functools.partial(_room, "B")),
    "roomA200": ("room", "A", functools.partial(_room, "A", 200)),  # partial last tile columns and rows on the faces
    "full": ("room", "A", _full),  # 2 x 6 + 4 = 16 light frames
}
FRAMES = {"T4": 4, "roomA": 8, "roomB": 8, "roomA200": 8, "full": 16}


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    scene, view, make = CASES[name]
    base = sc.case("T") if scene == "T" else oc.case(view)
    lights = make()
    assert sum(6 if l.kind == "point" else 1 for l in lights) == FRAMES[name]
    view_cam = sc.VIEW_CAM if scene == "T" else oc.VIEWS[view]
    return SimpleNamespace(name=name, scene=scene, view=base.view, view_cam=view_cam, n=base.n, offsets=base.offsets,
                           ids=base.ids, lights=lights)


def _vertices(scene: str) -> np.ndarray:
    return sc.scene_t_vertices() if scene == "T" else oc.room_vertices()


def _tag(values) -> str:
    """The values spelled out for a file name (-1.5 -> m1p5): one name per camera or origin, readable."""
    return "_".join(f"{v:g}".replace("-", "m").replace(".", "p") for v in values)


@functools.lru_cache(maxsize=None)
def _light_file(scene: str, cam: tuple) -> str:
    """The scene's triangles under a spot light's camera."""
    tag = _tag(cam)
    return sc.write_with_camera(sc._dir() / f"lighting_{scene}_{tag}.srt", _vertices(scene), cam)


@functools.lru_cache(maxsize=None)
def _point_case(view_path: str, origin: tuple) -> SimpleNamespace:
    """What omni_cases.restate reads of a case, for the room under a point light at `origin`."""
    tag = _tag(origin)
    faces = tuple(sc.write_with_camera(sc._dir() / f"lighting_room_{tag}_face{k}.srt", oc.room_vertices(),
                                       oc.face_camera(origin, k)) for k in range(6))
    return SimpleNamespace(view=view_path, faces=faces, origin=origin)


@functools.lru_cache(maxsize=None)
def _point_facts(name: str, origin: tuple, face_size: int):
    c = case(name)
    view = CASES[name][1]
    if origin == tuple(float(v) for v in oc.ORIGIN):
        return oc.facts(view, face_size)  # (shared with the omni tests)
    return oc.restate(_point_case(c.view, origin), face_size, c.offsets, c.ids)


@functools.lru_cache(maxsize=None)
def _spot_classes(scene: str, view_path: str, view: str | None, cam: tuple, wl: int, hl: int, bias: float) -> np.ndarray:
    if scene == "T":  # (shared with the shadow tests where they have the case)
        known = {(sc.LIGHT_CAM, sc.WL, sc.HL): "T", (sc.VIEW_CAM, W, H): "eye", (sc.AWAY_CAM, sc.WL, sc.HL): "away"}
        key = (tuple(float(v) for v in cam), wl, hl)
        for (kc, kw, kh), kname in known.items():
            if (tuple(float(v) for v in kc), kw, kh) == key:
                return sc.expected(kname, bias)
        base = sc.case("T")
    else:
        base = oc.case(view)
    m = sc.restate(view_path, _light_file(scene, cam), W, H, wl, hl, base.offsets, base.ids, bias)
    m.setflags(write=False)
    return m


def light_classes(name: str, light) -> np.ndarray:
    """The expected whole-frame class plane of one light of a case (read-only, once per session)."""
    c = case(name)
    if light.kind == "point":
        m = oc.mask_of(_point_facts(name, light.origin, light.face_size), c.ids, light.bias)
        m.setflags(write=False)
        return m
    return _spot_classes(c.scene, c.view, CASES[name][1], light.cam, light.wl, light.hl, light.bias)


def light_origin(name: str, light) -> np.ndarray:
    """The light's origin as the library holds it: the light frame's float32 origin."""
    if light.kind == "point":
        return np.array(light.origin, f32)
    s = oracle.OracleScene(_light_file(case(name).scene, light.cam))
    o = s.frame(light.wl, light.hl)[0:3].copy()
    s.close()
    return o


def dotv(a, b):
    """dotp on arrays of float32 triples: (a.x b.x + a.y b.y) + a.z b.z, one rounding per operation."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def frame_facts(view_path: str, w: int, h: int, off, ids=None) -> SimpleNamespace:
    """Steps 2 to 4 of the definition for every pixel of the file's w x h frame under the offsets
    `off` and the hit ids `ids` (None: the oracle's own render of the frame): surface, d, P, N, nn,
    nd, albedo (float32 arrays)."""
    s = oracle.OracleScene(view_path)
    n, ev, fv = s.n, s.edges(w, h), s.frame(w, h)
    v, alb, bg = s.vertices.astype(f32), s.albedo.astype(f32), s.background.astype(f32)
    with np.errstate(all="ignore"):
        ids = s.render(w, h, off)[..., 3].astype(np.int32) if ids is None else np.asarray(ids, np.int32)
    s.close()
    eye, base, du, dv = fv[0:3], fv[3:6], fv[6:9], fv[9:12]
    surface = (ids >= 0) & (ids < n)
    fx, fy, t = np.zeros((h, w), f32), np.zeros((h, w), f32), np.zeros((h, w), f32)
    for r in range(h):
        for x in range(w):
            px, py = oracle.pixel_position(x, r, float(off[r, x, 0]), float(off[r, x, 1]), w, h)
            fx[r, x], fy[r, x] = px, py
            if surface[r, x]:
                i = int(ids[r, x])
                hit, tt, _ = oracle.closest_hit(ev[i:i + 1], px, py)
                assert hit == 0
                t[r, x] = tt
    with np.errstate(all="ignore"):
        d = np.stack([(base[k] + fx * du[k]) + fy * dv[k] for k in range(3)], -1).astype(f32)
        p = np.stack([eye[k] + t * d[..., k] for k in range(3)], -1).astype(f32)
        e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
        normal = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                           e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(f32)
        safe = np.where(surface, ids, 0)
        nrm = normal[safe]
        out = SimpleNamespace(n=n, ids=ids, surface=surface, d=d, p=p, normal=nrm, nn=dotv(nrm, nrm), nd=dotv(nrm, d),
                              albedo=alb[safe], background=bg)
    for a in vars(out).values():
        if isinstance(a, np.ndarray):
            assert a.dtype in (f32, np.int32, np.bool_)
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def facts(view_path: str) -> SimpleNamespace:
    """frame_facts of a case's view: the 160 x 96 frame under the session's sample offsets and the
    oracle's ids."""
    return frame_facts(view_path, W, H, sc.random_offsets())


def terms(fa, cls, origin, light) -> SimpleNamespace:
    """Steps 6.1, 6.3 to 6.6 of one light for every pixel of frame_facts' frame, from the light's class
    plane and its float32 origin: q, qq, nl, facing, contributing, the weight w."""
    with np.errstate(all="ignore"):
        q = (fa.p - np.asarray(origin, f32)[None, None, :]).astype(f32)
        nl = dotv(fa.normal, q)
        facing = ((nl < 0) & (fa.nd < 0)) | ((nl > 0) & (fa.nd > 0))
        contributes = fa.surface & (cls == sc.LIT) & facing
        qq = dotv(q, q)
        cosine = np.abs(nl) / (np.sqrt(fa.nn) * np.sqrt(qq))
        cosl = np.where(cosine < 1, cosine, f32(1))
        w = cosl * (f32(light.falloff) / qq) if light.falloff > 0 else cosl
    assert w.dtype == f32
    return SimpleNamespace(cls=cls, q=q, qq=qq, nl=nl, facing=facing, contributes=contributes, w=w)


def light_terms(name: str, light) -> SimpleNamespace:
    """terms() of one light of a case."""
    return terms(facts(case(name).view), light_classes(name, light), light_origin(name, light), light)


def accumulate(fa, lights, per_light, ambient) -> np.ndarray:
    """The definition's accumulation for the whole frame: per_light[l] is terms() of lights[l]."""
    h, w = fa.ids.shape
    e = np.broadcast_to(np.array(ambient, f32), (h, w, 3)).copy()
    with np.errstate(all="ignore"):
        for light, lt in zip(lights, per_light):
            on = lt.contributes
            for k in range(3):
                e[..., k][on] = e[..., k][on] + f32(light.color[k]) * lt.w[on]  # (no + 0 for the others)
        out = np.empty((h, w, 4), f32)
        out[..., :3] = fa.albedo * e
    out[..., 3] = fa.ids.astype(f32)
    out[~fa.surface] = np.append(fa.background, f32(-1))
    return out


def restate_rgba(name: str, lights=None, ambient=AMBIENT) -> np.ndarray:
    """The definition for the whole frame under `lights` (default: the case's), in their order."""
    c = case(name)
    fa = facts(c.view)
    lights = c.lights if lights is None else lights
    assert np.array_equal(fa.ids, c.ids)
    return accumulate(fa, lights, [light_terms(name, light) for light in lights], ambient)


# --- the same restatement for any scene file, frame, offsets and ids (scale_cases) ----------------

@functools.lru_cache(maxsize=None)
def scene_light_file(path: str, cam: tuple) -> str:
    """The triangles of the scene file `path` under a spot light's camera."""
    from scenefile import read_scene, write_custom_scene

    _, bg, v, alb = read_scene(path)
    out = sc._dir() / f"{Path(path).stem}_{_tag(cam)}.srt"
    return write_custom_scene(out, v, alb, eye=cam[0:3], lookat=cam[3:6], up=cam[6:9], vfov=cam[9], background=bg)


@functools.lru_cache(maxsize=None)
def scene_point_case(path: str, origin: tuple) -> SimpleNamespace:
    """What omni_cases.restate reads of a case, for the scene file `path` under a point light."""
    from scenefile import read_scene, write_custom_scene

    _, bg, v, alb = read_scene(path)
    faces = []
    for k in range(6):
        cam = oc.face_camera(origin, k)
        faces.append(write_custom_scene(sc._dir() / f"{Path(path).stem}_{_tag(origin)}_face{k}.srt", v, alb, eye=cam[0:3],
                                        lookat=cam[3:6], up=cam[6:9], vfov=cam[9], background=bg))
    return SimpleNamespace(view=path, faces=tuple(faces), origin=origin)


def scene_light_facts(path: str, w: int, h: int, light, off, ids) -> SimpleNamespace:
    """What a light's class plane follows from at any bias: shadow_cases.restate_facts (a spot light) or
    omni_cases.restate (a point light) of the file's w x h frame."""
    if light.kind == "point":
        return oc.restate(scene_point_case(path, light.origin), light.face_size, off, ids, w=w, h=h)
    return sc.restate_facts(path, scene_light_file(path, light.cam), w, h, light.wl, light.hl, off, ids)


def scene_light_classes(light, light_facts, ids, bias=None) -> np.ndarray:
    bias = light.bias if bias is None else bias
    return (oc.mask_of if light.kind == "point" else sc.mask_of)(light_facts, ids, bias)


def scene_light_origin(path: str, light) -> np.ndarray:
    """light_origin for the scene file `path`."""
    if light.kind == "point":
        return np.array(light.origin, f32)
    s = oracle.OracleScene(scene_light_file(path, light.cam))
    o = s.frame(light.wl, light.hl)[0:3].copy()
    s.close()
    return o


def restate_frame(path: str, w: int, h: int, lights, ambient, off, ids, fa=None, light_facts=None) -> SimpleNamespace:
    """The definition for the w x h frame of the scene file `path` under `lights`, the sample offsets
    `off` and the hit ids `ids`: the class planes (L, h, w), the RGBA (h, w, 4), and what they follow
    from (fa: frame_facts; light_facts and terms: one entry per light), which a caller may hand back
    in to spare their recomputation (they do not depend on colour, falloff or bias)."""
    fa = frame_facts(path, w, h, off, ids) if fa is None else fa
    if light_facts is None:
        light_facts = [scene_light_facts(path, w, h, l, off, ids) for l in lights]
    classes = [scene_light_classes(l, f, ids) for l, f in zip(lights, light_facts)]
    per_light = [terms(fa, cls, scene_light_origin(path, l), l) for l, cls in zip(lights, classes)]
    return SimpleNamespace(classes=np.stack(classes) if lights else np.empty((0, h, w), np.uint8),
                           rgba=accumulate(fa, lights, per_light, ambient), fa=fa, light_facts=light_facts,
                           terms=per_light)


def expected_classes(name: str, lights=None) -> np.ndarray:
    c = case(name)
    lights = c.lights if lights is None else lights
    return np.stack([light_classes(name, l) for l in lights]) if lights else np.empty((0, H, W), np.uint8)


@functools.lru_cache(maxsize=None)
def expected(name: str) -> SimpleNamespace:
    """The case's expected class planes (L, H, W) and RGBA (H, W, 4) under AMBIENT (read-only)."""
    out = SimpleNamespace(classes=expected_classes(name), rgba=restate_rgba(name))
    out.classes.setflags(write=False)
    out.rgba.setflags(write=False)
    return out


def light_counts(name: str, light) -> SimpleNamespace:
    lt = light_terms(name, light)
    lit = lt.cls == sc.LIT
    return SimpleNamespace(classes=sc.counts(lt.cls), contributing=int(lt.contributes.sum()),
                           lit_not_facing=int((lit & ~lt.facing).sum()))


def check_expected(name: str):
    """What keeps a test from passing vacuously. Counts out of 15 360 pixels (CPU, oracle
    restatement): T under LIGHT_CAM classes (383, 3471, 2302, 9204), 3381 contributing, 90 lit but not
    facing; T under BELOW_CAM 0 contributing, every class-1 pixel not facing; room A / B under
    SPOT_IN 5186 / 6002 contributing, 667 / 141 lit but not facing; under the point light at
    F = 64 12383 / 11581 and 260 / 921. The second point light of "full" (ORIGIN2, F = 64, bias 0):
    classes (1029, 14331, 0, 0), 14290 contributing, 41 lit but not facing: the 1 % rule holds."""
    c = case(name)
    for k, light in enumerate(c.lights):
        cam = getattr(light, "cam", None)
        got = light_counts(name, light)
        what = f"{name} light {k}: classes {got.classes}, {got.contributing} contributing, {got.lit_not_facing} lit not facing"
        if cam == tuple(float(v) for v in sc.AWAY_CAM):
            assert got.classes[0] == got.classes[1] == 0 and got.classes[2] > 1000, what
            continue
        if cam == BELOW_CAM:
            assert got.contributing == 0 and got.classes[1] >= 1000 and got.lit_not_facing == got.classes[1], what
            continue
        assert got.contributing >= (W * H) // 100, what
        is_head = cam == tuple(float(v) for v in c.view_cam)
        if is_head:  # q = t d: every surface pixel is lit and facing
            assert got.contributing == got.classes[1] and got.classes[0] == 0 and got.lit_not_facing == 0, what
        if cam == tuple(float(v) for v in sc.LIGHT_CAM):
            assert min(got.classes) >= (W * H) // 50 and got.lit_not_facing >= 50, what
        if c.scene == "room" and not is_head and k < 2:  # the room's point light and SPOT_IN
            assert got.lit_not_facing >= 50, what


def host_lights(lights):
    from simpleraytracer_amd import PointLightHost, SpotLightHost

    return [PointLightHost(l.origin, l.face_size, l.color, l.falloff, l.bias) if l.kind == "point" else
            SpotLightHost(l.cam, l.wl, l.hl, l.color, l.falloff, l.bias) for l in lights]


def same_bits(name, got, want):
    sc.same_bits(name, got, want)


same_bits_or_nan = sc.same_bits_or_nan


def assert_same_classes(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape, got.dtype)
    for k in range(got.shape[0]):
        sc.assert_same_mask(got[k], want[k])
