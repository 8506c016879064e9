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
