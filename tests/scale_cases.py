"""Shared cases of the coordinate-range tests (test_scale_host.py, test_gpu_scale.py): scenes whose
coordinates, view angle and frame aspect leave the regime of every other test (coordinates of order
1, a 15 to 110 degree view, frames near 16:9), and the oracle's answers. Not a test module.

Scene S is query_cases' scene Q geometry (a soup, triangles behind the eye, two degenerate and two
frame-covering triangles) with a random albedo, under a camera whose numbers are dyadic, written
after multiplying vertices, eye and look-at by 2^k. The scaling is exact in float32, and so is every
expression of DESIGN.md section 2 under it: the camera frame is normalised in double on the host,
eye-relative vertices scale by s = 2^k, edge coefficients by s^2, vol by s^3, t = vol / det by s. So
the oracle's ids are those of k = 0, t is t0 2^k and RGB is that of k = 0 while the shading normal's
n . n (s^4) stays inside the float range. What changes with k is the path the library takes: the
record pass solves a screen box in float only while every coefficient lies in [2^-40, 2^30]
(csrc/screen_box.h), else in double; the slack and the pads carry absolute terms.

Scene C ("cloud") is 1 500 small triangles in [-1, 1]^3 seen by telephoto cameras far away (boxes of
many screens: the quantisation clamp, the large list), by fisheye cameras inside it (triangles all
round and behind the eye: unbounded boxes, huge du), in strip-shaped frames and under a rolled up
vector.

Every case's conditions are asserted on the oracle's answers here (guards), so no test of a case
passes vacuously. Files and answers are made once per session and shared read-only.
"""
from __future__ import annotations

import atexit
import ctypes
import functools
import shutil
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import layers_cases as lc
import query_cases as qc
from oracle import srt_oracle as oracle
from scenefile import write_custom_scene

f32 = np.float32
W, H = 200, 72  # 4 x 5 tiles of 64 x 16: a last tile column of 8 pixels, a last tile row of 8 rows
BACKGROUND = (0.1, 0.2, 0.3)
S_EYE, S_LOOK, S_UP, S_VFOV = (0.125, -0.25, 0.0), (0.25, 0.125, 3.0), (0.0, 1.0, 0.0), 60.0
SHIFTS = {"shift": (4096.0, -2048.0, 8192.0), "shift_far": (1e5, 3e5, -2e5)}
HOST_KS = (-30, -21, -16, -15, -8, 0, 8, 14, 15, 16, 21, 30)
LAYERS = 4
T_EXACT_K, RGB_EXACT_K = 30, 20  # |k| up to which t / 2^k, and RGB, are those of k = 0 on the bits

N_CLOUD = 1500
INSIDE = ((0.05, 0.02, 0.01), (0.3, 0.1, 1.0))  # an eye inside the cloud
ORIGIN = (0.0, 0.0, 0.0)
# name -> (eye, look-at, up, vfov, W, H)
CLOUD = {
    "tele200": ((0.3, 0.2, -200.0), ORIGIN, S_UP, 0.8, W, H),
    "tele2000": ((30.0, 20.0, -2000.0), ORIGIN, S_UP, 0.08, W, H),
    "tele2e4": ((300.0, 200.0, -20000.0), ORIGIN, S_UP, 0.008, W, H),
    "fish170": (*INSIDE, S_UP, 170.0, W, H),
    "fish179": (*INSIDE, S_UP, 179.0, W, H),
    "fish179_9": (*INSIDE, S_UP, 179.9, W, H),
    "wide": (*INSIDE, S_UP, 60.0, 2000, 8),
    "wide4100": (*INSIDE, S_UP, 60.0, 4100, 3),
    "tall": ((0.05, 0.02, -3.0), ORIGIN, S_UP, 120.0, 8, 2000),
    "rolled": ((2.0, 1.0, -2.5), ORIGIN, (0.7, 0.1, 0.7), 45.0, W, H),
}
CLOUD_NAMES = tuple(CLOUD)
EXTRA_NAMES = ("fov1", "shift", "shift_far")


def s_name(k: int) -> str:
    return f"k{k}"


@functools.lru_cache(maxsize=None)
def _dir() -> Path:
    d = tempfile.mkdtemp(prefix="scale_cases_")
    atexit.register(shutil.rmtree, d, True)
    return Path(d)


@functools.lru_cache(maxsize=None)
def s_geometry():
    """(vertices (424, 3, 3) float32, albedo (424, 3) float32): Q's geometry, the albedo drawn after
    it from the same generator."""
    rng = np.random.default_rng(11)
    v = qc.scene_q_vertices(rng)
    albedo = rng.uniform(0.2, 1.0, (len(v), 3)).astype(f32)
    for a in (v, albedo):
        a.setflags(write=False)
    return v, albedo


def scaled_camera(eye, look, k: int = 0, shift=None):
    """(eye, look-at) float32: + shift in float32 (inexact), then times 2^k (exact)."""
    s = f32(2.0) ** k
    e, l = np.asarray(eye, f32), np.asarray(look, f32)
    if shift is not None:
        e, l = e + np.asarray(shift, f32), l + np.asarray(shift, f32)
    assert e.dtype == f32 and np.all(np.isfinite(e * s)) and np.all(((e * s) / s) == e)
    return e * s, l * s


def write_s(path, k: int = 0, shift=None, vfov: float = S_VFOV) -> str:
    """Scene S: the float32 geometry, plus `shift` (a float32 vector, float32 additions), times 2^k."""
    v, albedo = s_geometry()
    v = np.array(v)
    if shift is not None:
        v = v + np.asarray(shift, f32)
    s = f32(2.0) ** k
    scaled = v * s
    assert scaled.dtype == f32 and np.array_equal(scaled / s, v)  # exact
    eye, look = scaled_camera(S_EYE, S_LOOK, k, shift)
    return write_custom_scene(path, scaled.reshape(-1, 9), albedo, eye=eye, lookat=look, up=S_UP, vfov=vfov,
                              background=BACKGROUND)


@functools.lru_cache(maxsize=None)
def cloud_geometry():
    rng = np.random.default_rng(21)
    centre = rng.uniform(-1, 1, (N_CLOUD, 3))
    v = (centre[:, None, :] + rng.uniform(-0.12, 0.12, (N_CLOUD, 3, 3))).astype(f32)
    albedo = rng.uniform(0.2, 1, (N_CLOUD, 3)).astype(f32)
    return v, albedo


def write_cloud(path, name: str) -> str:
    eye, look, up, vfov, _, _ = CLOUD[name]
    v, albedo = cloud_geometry()
    return write_custom_scene(path, v.reshape(-1, 9), albedo, eye=eye, lookat=look, up=up, vfov=vfov,
                              background=BACKGROUND)


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    """A case by name: 'k<k>' (scene S times 2^k), 'fov1', 'shift', 'shift_far', or a cloud camera.
    (name, path, w, h, k): k is None where the case is not a scaled S."""
    path = _dir() / f"{name}.srt"
    w, h, k = W, H, None
    if name in CLOUD:
        write_cloud(path, name)
        w, h = CLOUD[name][4:6]
    elif name == "fov1":
        write_s(path, vfov=1.0)
    elif name in SHIFTS:
        write_s(path, shift=SHIFTS[name])
    else:
        assert name.startswith("k"), name
        k = int(name[1:])
        write_s(path, k)
    return SimpleNamespace(name=name, path=str(path), w=w, h=h, k=k)


def offsets(w: int, h: int) -> np.ndarray:
    return np.random.default_rng(3).random((h, w, 2), f32)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, f32).view(np.uint32)


def enabled_records(name: str) -> np.ndarray:
    """The oracle's edge records (c0, cx, cy per edge: 9 floats) of the triangles it did not disable."""
    c = case(name)
    sc = oracle.OracleScene(c.path)
    e = sc.edges(c.w, c.h)
    sc.close()
    return np.ascontiguousarray(e[~np.isnan(e[:, 9]), :9])


def host_box(rec9, mode: int):
    """srtScreenBoxHost: (answered, (xlo, xhi, ylo, yhi)); mode 0 the solve the record pass takes, 1
    the double solve, 2 the float solve (not answered: the record takes the double one)."""
    from simpleraytracer_amd import _native

    arr = (ctypes.c_float * 9)(*[float(v) for v in rec9])
    out = (ctypes.c_float * 4)()
    return _native.lib().srtScreenBoxHost(arr, mode, out) == 0, tuple(out)


@functools.lru_cache(maxsize=None)
def float_share(name: str) -> float:
    """The share of the case's enabled records whose screen box the float solve answers."""
    recs = enabled_records(name)
    assert len(recs) >= 400
    return float(np.mean([host_box(r, 2)[0] for r in recs]))


def assert_float_share(k: int):
    share = float_share(s_name(k))
    if k in (-8, 0, 8, 14):
        assert share >= 0.90, (k, share)
    elif k == 15:
        assert 0.10 <= share <= 0.60, (k, share)
    elif abs(k) >= 16:
        assert share <= 0.02, (k, share)


@functools.lru_cache(maxsize=None)
def frame(name: str, kind: str = "rnd") -> np.ndarray:
    """The oracle's frame of a case: kind 'rnd' (offsets()) or 'half' (uniform 0.5). The case's guards
    are asserted on the 'rnd' frame."""
    c = case(name)
    sc = oracle.OracleScene(c.path)
    with np.errstate(all="ignore"):
        out = sc.render(c.w, c.h, offsets(c.w, c.h) if kind == "rnd" else None)
    sc.close()
    out.setflags(write=False)
    if kind == "rnd":
        _guard_frame(c, out)
    return out


def _guard_frame(c, fr):
    ids = fr[..., 3]
    hit = float((ids >= 0).mean())
    distinct = len(np.unique(ids[ids >= 0]))
    if c.name in CLOUD:
        assert hit >= 0.1 and distinct >= (10 if c.name == "wide4100" else 50), (c.name, hit, distinct)
    elif c.name == "fov1":
        assert hit >= 0.1, (c.name, hit)
        boxes = [host_box(r, 0) for r in enabled_records(c.name)]
        assert all(ok for ok, _ in boxes)
        assert any(max(abs(v) for v in b) > 8 for _, b in boxes), "fov1: no screen box beyond +-8"
    elif c.name in SHIFTS:
        assert hit >= 0.1 and distinct >= 50, (c.name, hit, distinct)
    elif c.k == 0:
        assert 0.3 <= hit <= 0.7, hit
        assert np.isin(ids, qc.LARGE_IDS).mean() >= 0.20
        assert distinct >= 150, distinct
        assert_float_share(0)
    else:
        f0 = frame(s_name(0))
        assert np.array_equal(bits(ids), bits(f0[..., 3])), f"k = {c.k}: the oracle's ids are not those of k = 0"
        if abs(c.k) <= RGB_EXACT_K:
            assert np.array_equal(bits(fr[..., :3]), bits(f0[..., :3])), f"k = {c.k}: the oracle's RGB is not that of k = 0"
        assert_float_share(c.k)


def scaled_t(t0: np.ndarray, k: int) -> np.ndarray:
    """t0 2^k in float32 (exact for |k| <= 30 on scene S: no result leaves the normal range)."""
    out = np.asarray(t0, f32) * (f32(2.0) ** k)
    assert out.dtype == f32
    return out


@functools.lru_cache(maxsize=None)
def answers(name: str):
    """(pos, ids, t): the oracle's closest hit at query_cases.mixed_positions of the case's frame. On
    a scaled S: ids those of k = 0, t = t0 2^k on the bits."""
    c = case(name)
    frame(name)  # the guards
    pos = qc.mixed_positions(c.w, c.h)
    ids, t = qc.oracle_answers(c.path, c.w, c.h, pos)
    for a in (pos, ids, t):
        a.setflags(write=False)
    assert (ids >= 0).sum() >= 0.05 * len(ids) and (ids < 0).sum() >= 0.05 * len(ids), name
    if c.k not in (None, 0):
        _, ids0, t0 = answers(s_name(0))
        assert np.array_equal(ids, ids0), f"k = {c.k}: the oracle's ids at the positions are not those of k = 0"
        if abs(c.k) <= T_EXACT_K:
            assert np.array_equal(bits(t), bits(scaled_t(t0, c.k))), f"k = {c.k}: the oracle's t is not t0 2^k"
    return pos, ids, t


@functools.lru_cache(maxsize=None)
def layers(name: str, key: str = "mixed"):
    """(pos, ids (4, count), t (4, count)): layers_cases' peel of the oracle's closest hit, K = 4, at
    the mixed positions or ('pixels') at the frame's pixels under offsets(). Layer 0 is answers()'."""
    c = case(name)
    if key == "mixed":
        pos, ids0, t0 = answers(name)
    else:
        pos = lc.pixel_positions(c.w, c.h, offsets(c.w, c.h))
    ids, t = lc.oracle_layers(c.path, c.w, c.h, pos, LAYERS)
    for a in (pos, ids, t):
        a.setflags(write=False)
    if key == "mixed":
        lc.assert_same(ids[0], t[0], ids0, t0)
    else:
        assert np.array_equal(ids[0].reshape(c.h, c.w).astype(f32), frame(name)[..., 3])
    assert (ids[LAYERS - 1] >= 0).any(), f"{name}: no position with {LAYERS} hits"
    return pos, ids, t


# Shadow: scene S under a light to the right of and above the eye that looks across the soup at the
# covering triangles; eye and look-at scale with the scene, every number dyadic.
LIGHT_EYE, LIGHT_LOOK, LIGHT_UP, LIGHT_VFOV = (3.0, 2.0, 1.0), (-1.5, -0.5, 9.0), (0.0, 1.0, 0.0), 40.0
LIGHT_W, LIGHT_H = 192, 80
SHADOW_BIASES = (0.0, 0.25)


def light_camera(k: int = 0):
    eye, look = scaled_camera(LIGHT_EYE, LIGHT_LOOK, k)
    return (*[float(v) for v in eye], *[float(v) for v in look], *LIGHT_UP, LIGHT_VFOV)


def frame_ids(name: str) -> np.ndarray:
    """The oracle's hit ids (H, W) int32 of the case's 'rnd' frame."""
    fr = frame(name)
    ids = fr[..., 3].astype(np.int32)
    assert np.array_equal(ids.astype(f32), fr[..., 3])
    return ids


def assert_shadow_classes(mask):
    """The k = 0 mask holds shadowed, lit and outside-the-frustum pixels, 2 % of the frame each."""
    counts = [int((np.asarray(mask) == c).sum()) for c in range(3)]
    assert all(n >= 0.02 * np.asarray(mask).size for n in counts), f"degenerate light: class counts {counts}"


# Lights, surfaces and materials (rto*, rtd*, rtv*, rtp*): what these families compute after the hit,
# across scale and at the edges of float32.
#
# The rig of S times 2^k: the spot light above, a second one on the other side of S, and a point light
# at the first one's eye, every position times 2^k; count_cases' colours and ambient. c of "Lighting"
# is scale-free (nl ~ s^3, sqrt(nn) ~ s^2, sqrt(qq) ~ s, every factor a power of two); the falloffs are
# (0, f1 4^k, f2 4^k), so that falloff / qq is too: the lit frame of S times 2^k has the bits of k = 0
# while nn = N . N (s^4) stays a normal number. It does not at k = -30 (nn of S's small triangles is
# subnormal, or 0) and at k = +30 (nn of the two covering triangles is +inf: c = 0, they go dark);
# there the frame is compared at its own k only. The bias is relative (thr = z - b z), so the masks at
# bias 0 are those of k = 0; the run with the bias RIG_BIAS 2^k is not scale-free and probes b z.
#
# The surface tables do not scale: weights, uv and the normal plane are scale-free. The magnitude
# sweep multiplies the normals table by 2^m at k = 0, so that Ns . Ns of "Vertex attributes" is 0,
# subnormal, ordinary, huge and +inf.
#
# The library refuses a point light's origin beyond |o_k| <= 2^16 (DESIGN.md section 2 "Omni shadow":
# fl32(o + axis) must stay a direction), and the first spot light's eye is (3, 2, 1) 2^k: the rig holds
# the point light up to k = 14, which therefore stands beside 16 among the large scales, and at k = 16
# and 30 the tests assert the refusal and light the scene with the two spot lights.
#
# Counts obtained (CPU, numpy; conditions on the inputs, asserted with their thresholds by
# test_scale_host.test_rig_guards and test_sweep_and_shininess_guards). 14 400 pixels, 7 534 of them hit:
#   k = 0     light 0 (spot): 518 shadowed, 4 402 lit, 4 295 contributing (thresholds 100, 100)
#             light 1 (spot): 195 shadowed, 2 249 lit, 2 061 contributing
#             light 2 (point): 659 shadowed, 6 875 lit, 6 628 contributing
#             4 669 hit pixels (62 %) under two or more lights (threshold: a fifth)
#   k = -30   12 984 (lit pixel, light) pairs, nn nonzero subnormal in 1 398 (10.8 %; threshold 5 %);
#             nn == 0 in 0: S yields none (its two degenerate triangles are never hit)
#   k = +30   nn == +inf at 6 356 pixels (threshold 100): the covering triangles, dark but for the ambient
#   normals table times 2^m: Ns . Ns is 0 at all 7 534 hit pixels for m = -75 (threshold 100), nonzero
#             subnormal at all of them for m = -64 (threshold 5 %), ordinary for m = 0, finite for m = 63,
#             +inf at 131 pixels for m = 64 (threshold 100)
#   shininess_log2 = 12: s^4096 is a nonzero subnormal in 470 (pixel, light) pairs (threshold 16; table
#             seeds 1 .. 79 give 1 to 1 089, seed 27 of test_gpu_surface.py gives 4); under the black
#             texture 196 pixels hold a subnormal rgb value
LIGHT2_EYE, LIGHT2_LOOK, LIGHT2_VFOV = (-3.0, 1.5, 0.5), (1.5, 0.5, 9.0), 50.0
FACE = 64
RIG_KS = (-30, -21, 0, 14, 16, 30)  # (the point light's origin is accepted up to k = 14: 3 x 2^14 <= 2^16)
RIG_FALLOFF = (0.0, 16.0, 8.0)  # times 4^k
RIG_BIAS = 0.25                 # times 2^k, in the biased run
TABLE_SEED, TEXTURE_SEED, TEXTURE = 12, 11, (3, 5)  # (of seeds 1 .. 79 the table with the most subnormal highlights)
SWEEP_MS = (-75, -64, 0, 63, 64)
SPECULAR = (0.9, 0.7, 0.5)
SHININESS = (0, 1, 12)


def light2_camera(k: int = 0):
    eye, look = scaled_camera(LIGHT2_EYE, LIGHT2_LOOK, k)
    return (*[float(v) for v in eye], *[float(v) for v in look], *LIGHT_UP, LIGHT2_VFOV)


def point_origin(k: int = 0):
    return tuple(float(v) for v in scaled_camera(LIGHT_EYE, LIGHT_LOOK, k)[0])


def point_allowed(k: int) -> bool:
    """DESIGN.md section 2 "Omni shadow": a point light's origin is refused beyond |o_k| <= 2^16."""
    return max(abs(v) for v in point_origin(k)) <= 65536.0


def rig(k: int = 0, biased: bool = False, point: bool | None = None):
    """The lights of S times 2^k (lighting_cases.spot / point): spot, spot and -- point=None: where
    the library accepts its origin -- the point light."""
    import count_cases as cc
    import lighting_cases as lt

    f = [float(np.ldexp(f32(v), 2 * k)) for v in RIG_FALLOFF]
    bias = float(np.ldexp(f32(RIG_BIAS), k)) if biased else 0.0
    lights = [lt.spot(light_camera(k), LIGHT_W, LIGHT_H, cc.LIGHT_COLORS[0], f[0], bias),
              lt.spot(light2_camera(k), LIGHT_W, LIGHT_H, cc.LIGHT_COLORS[1], f[1], bias)]
    if point_allowed(k) if point is None else point:
        assert point_allowed(k), k
        lights.append(lt.point(point_origin(k), FACE, cc.LIGHT_COLORS[2], f[2], bias))
    return lights


def ambient():
    import count_cases as cc

    return cc.AMBIENT


@functools.lru_cache(maxsize=None)
def _rig_facts(k: int):
    """(frame_facts, [light facts]) of S times 2^k under rig(k): what every run at k shares."""
    import lighting_cases as lt

    c = case(s_name(k))
    off, ids = offsets(W, H), frame_ids(c.name)
    return (lt.frame_facts(c.path, W, H, off, ids),
            [lt.scene_light_facts(c.path, W, H, light, off, ids) for light in rig(k)])


@functools.lru_cache(maxsize=None)
def lit(k: int, biased: bool = False, point: bool | None = None) -> SimpleNamespace:
    """lighting_cases.restate_frame of S times 2^k under rig(k, biased, point): classes, rgba, fa,
    terms (read-only, once per session)."""
    import lighting_cases as lt

    c = case(s_name(k))
    fa, light_facts = _rig_facts(k)
    lights = rig(k, biased, point)
    out = lt.restate_frame(c.path, W, H, lights, ambient(), offsets(W, H), frame_ids(c.name), fa=fa,
                           light_facts=light_facts[:len(lights)])
    for a in (out.classes, out.rgba):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pixel_edges(k: int) -> SimpleNamespace:
    """surface_cases.edge_values of every pixel of the frame of S times 2^k, in row order."""
    import surface_cases as sv

    c = case(s_name(k))
    return sv.edge_values(c.path, W, H, lc.pixel_positions(W, H, offsets(W, H)), frame_ids(c.name).reshape(-1))


@functools.lru_cache(maxsize=None)
def surface_tables() -> SimpleNamespace:
    """surface_cases.tables for S (the planted uvs on triangles the frame hits) and a 3 x 5 texture."""
    import surface_cases as sv

    tb = sv.tables(len(s_geometry()[0]), TABLE_SEED, hit_ids=frame_ids(s_name(0)).reshape(-1))
    tb.texture = sv.texture(*TEXTURE, TEXTURE_SEED)
    return tb


@functools.lru_cache(maxsize=None)
def surface(m: int = 0, wrap: str = "repeat", filter: str = "bilinear"):
    """The Surface of numpy tables: the normals table times 2^m (float32), uvs and the texture."""
    from simpleraytracer_amd import Surface

    tb = surface_tables()
    with np.errstate(all="ignore"):
        normals = (tb.normals * f32(2.0) ** m).astype(f32) if m else tb.normals
    normals.setflags(write=False)
    return Surface(normals, tb.uvs, tb.texture, wrap, filter)


@functools.lru_cache(maxsize=None)
def surface_planes(k: int, m: int = 0, wrap: str = "repeat", filter: str = "bilinear") -> SimpleNamespace:
    """surface_cases.expected of the frame of S times 2^k under surface(m, wrap, filter)."""
    import surface_cases as sv

    s = surface(m, wrap, filter)
    return sv.expected(pixel_edges(k), s.normals, s.uvs, s.texture, wrap, filter)


@functools.lru_cache(maxsize=None)
def black_surface():
    """surface() with a black 1 x 1 texture: the albedo plane is 0, so a lit pixel is its highlight alone
    (specular . S) and a subnormal S, which any albedo . E of ordinary size absorbs, reaches the output."""
    from simpleraytracer_amd import Surface

    tb = surface_tables()
    black = np.zeros((1, 1, 4), f32)
    black.setflags(write=False)
    return Surface(tb.normals, tb.uvs, black)


def lit_surface(k: int, m: int = 0, material=None, point: bool | None = None, black: bool = False) -> np.ndarray:
    """litsurface_cases' restatement of S times 2^k under rig(k, point=point) and surface(m), or
    black_surface(): (H, W, 4) float32."""
    import litsurface_cases as pc

    base = lit(k, False, point)
    return pc.accumulate(base.fa, pixel_edges(k), rig(k, False, point), base.terms, ambient(),
                         black_surface() if black else surface(m), material)


def check_planes(what: str, got: dict, exp):
    """The four planes of a surface call against surface_cases.expected, on the bits (a NaN for a NaN)."""
    from shadow_cases import same_bits_or_nan

    for name in ("uv", "albedo", "normal", "rgba"):
        same_bits_or_nan(f"{what}: {name}", np.asarray(got[name]).reshape(-1, got[name].shape[-1]), getattr(exp, name))


def table_nn(m: int) -> np.ndarray:
    """dotp(Ns, Ns) of the hit pixels of the k = 0 frame under the normals table times 2^m."""
    import surface_cases as sv

    ev = pixel_edges(0)
    ns = sv.interpolate(ev, surface(m).normals)
    return sv.dotp(ns, ns)[ev.valid]


def subnormal(a) -> np.ndarray:
    """Nonzero and below the smallest normal float32."""
    a = np.abs(np.asarray(a, f32))
    return (a > 0) & (a < np.finfo(f32).tiny)


def highlights(k: int, shininess_log2: int):
    """(s, shines) per light: litsurface_cases.highlight under surface(0), and where it is added."""
    import lighting_cases as lt
    import litsurface_cases as pc

    fa = lit(k).fa
    u = surface_planes(k).normal[:, :3].reshape(H, W, 3)
    out = []
    with np.errstate(all="ignore"):
        for light, t in zip(rig(k), lit(k).terms):
            w = pc.falloff(pc.clamp01((f32(0) - lt.dotv(u, t.q)) / np.sqrt(t.qq)), t.qq, light)
            out.append((pc.highlight(fa, u, t.q, t.qq, shininess_log2), t.contributes & (w > 0)))
    return out
