"""Shared cases of the shadow-mask tests (test_shadow_host.py, test_gpu_shadow.py): the scenes, the
numpy float32 restatement of DESIGN.md section 2 "Shadow" and the expected masks -- from the oracle
and numpy, never from the library. Not a test module.

Expected values: the view file's and a light file's (the same triangles under the light's camera,
write_custom_scene) OracleScene.edges / frame, oracle.pixel_position, oracle.closest_hit, and the
steps of the definition in numpy float32, one rounding per operation. The hit ids are the oracle's
own render of the view frame. A case's files and expected masks are computed once per session and
shared read-only.
"""
from __future__ import annotations

import atexit
import functools
import shutil
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from oracle import srt_oracle as oracle
from scenefile import write_custom_scene

f32 = np.float32
SHADOWED, LIT, OUTSIDE, NO_SURFACE = 0, 1, 2, 3
BIASES = (0.0, 2.0 ** -10)

W, H = 160, 96
VIEW_CAM = (0.0, 1.5, -1.0, 0.0, -1.0, 4.0, 0.0, 1.0, 0.0, 60.0)
LIGHT_CAM = (1.0, 4.0, 3.0, 0.0, -1.0, 4.0, 0.0, 0.0, 1.0, 50.0)
AWAY_CAM = (1.0, 4.0, 3.0, 1.0, 9.0, 3.5, 0.0, 0.0, 1.0, 50.0)  # looks up, away from everything
WL, HL = 192, 80  # 3 x 5 tiles of 64 x 16


def _quad_y(y, x0, x1, z0, z1):
    a, b, c, d = (x0, y, z0), (x1, y, z0), (x1, y, z1), (x0, y, z1)
    return [[a, b, c], [a, c, d]]


def scene_t_vertices() -> np.ndarray:
    """Scene T: a floor quad, an occluder quad above it and 200 soup triangles around both."""
    rng = np.random.default_rng(7)
    c = rng.uniform([-2.0, -0.8, 2.0], [2.0, 0.5, 6.0], (200, 3))
    soup = c[:, None, :] + rng.uniform(-0.15, 0.15, (200, 3, 3))
    floor = _quad_y(-1.0, -3.0, 3.0, 1.0, 7.0)
    occluder = _quad_y(0.0, -0.5, 0.5, 3.5, 4.5)
    return np.concatenate([np.array(floor), np.array(occluder), soup]).astype(f32).reshape(-1, 9)


def grid_floor_vertices(cells: int = 12) -> np.ndarray:
    """The floor of scene T as cells x cells quads: coplanar neighbours across every mesh edge."""
    xs = np.linspace(-3.0, 3.0, cells + 1)
    zs = np.linspace(1.0, 7.0, cells + 1)
    tris = []
    for i in range(cells):
        for j in range(cells):
            tris += _quad_y(-1.0, xs[i], xs[i + 1], zs[j], zs[j + 1])
    return np.array(tris).astype(f32).reshape(-1, 9)


# name -> (vertices, light camera, light frame)
CASES = {
    "T": (scene_t_vertices, LIGHT_CAM, (WL, HL)),
    "T200": (scene_t_vertices, LIGHT_CAM, (200, 72)),  # a partial last tile column and row
    "eye": (scene_t_vertices, VIEW_CAM, (W, H)),       # the light at the eye
    "grid": (grid_floor_vertices, LIGHT_CAM, (WL, HL)),
    "away": (scene_t_vertices, AWAY_CAM, (WL, HL)),
}


@functools.lru_cache(maxsize=None)
def _dir() -> Path:
    d = tempfile.mkdtemp(prefix="shadow_cases_")
    atexit.register(shutil.rmtree, d, True)
    return Path(d)


def _albedo(n: int) -> np.ndarray:
    return np.random.default_rng(23).uniform(0.2, 1.0, (n, 3)).astype(f32)


def write_with_camera(path, vertices, cam, background=(0.1, 0.2, 0.3)) -> str:
    return write_custom_scene(path, vertices, _albedo(len(vertices)), eye=cam[0:3], lookat=cam[3:6], up=cam[6:9],
                              vfov=cam[9], background=background)


def random_offsets(seed: int = 3) -> np.ndarray:
    return np.random.default_rng(seed).random((H, W, 2), dtype=f32)


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    """The case's files, the view frame's sample offsets and the oracle's hit ids of them."""
    make, light_cam, (wl, hl) = CASES[name]
    v = make()
    view = write_with_camera(_dir() / f"{name}_view.srt", v, VIEW_CAM)
    light = write_with_camera(_dir() / f"{name}_light.srt", v, light_cam)
    off = random_offsets()
    sc = oracle.OracleScene(view)
    ids = sc.render(W, H, off)[..., 3].astype(np.int32)
    sc.close()
    for a in (off, ids):
        a.setflags(write=False)
    return SimpleNamespace(name=name, view=view, light=light, light_cam=light_cam, wl=wl, hl=hl, n=len(v), offsets=off,
                           ids=ids)


def projection_rows(frame12: np.ndarray) -> np.ndarray:
    """(px, py, pz) of a light frame (origin, base, du, dv: float32), in float64 with + - x / only,
    in the definition's order, each component rounded once to float32: (3, 3) float32."""
    fr = np.asarray(frame12, f32).astype(np.float64)
    base, du, dv = fr[3:6], fr[6:9], fr[9:12]

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    f = (base + 0.5 * du) + 0.5 * dv
    px = du / dot(du, du) + 0.5 * f
    py = dv / dot(dv, dv) + 0.5 * f
    return np.stack([px, py, f]).astype(f32)


def dotp(a, b) -> np.float32:
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def restate_facts(view: str, light: str, w: int, h: int, wl: int, hl: int, offsets, ids, row_begin: int = 0):
    """The definition up to the bias, pixel by pixel, for the band whose offsets and ids are given:
    surface (the id lies inside the scene), outside (class 2), z and the light frame's closest hit
    (li, lt)."""
    sv, sl = oracle.OracleScene(view), oracle.OracleScene(light)
    n = sv.n
    assert sl.n == n
    ev, el = sv.edges(w, h), sl.edges(wl, hl)
    fv, fl = sv.frame(w, h), sl.frame(wl, hl)
    sv.close()
    sl.close()
    eye, base, du, dv = fv[0:3], fv[3:6], fv[6:9], fv[9:12]
    lorigin = fl[0:3]
    px, py, pz = projection_rows(fl)
    rows = ids.shape[0]
    out = SimpleNamespace(surface=np.zeros((rows, w), bool), outside=np.zeros((rows, w), bool),
                          z=np.zeros((rows, w), f32), li=np.full((rows, w), -1, np.int64),
                          lt=np.full((rows, w), np.inf, f32))
    with np.errstate(all="ignore"):
        for r in range(rows):
            for x in range(w):
                i = int(ids[r, x])
                if not 0 <= i < n:
                    continue
                out.surface[r, x] = True
                fx, fy = oracle.pixel_position(x, row_begin + r, float(offsets[r, x, 0]), float(offsets[r, x, 1]), w, h)
                hit, t, _ = oracle.closest_hit(ev[i:i + 1], fx, fy)
                assert hit == 0, f"pixel ({x}, {row_begin + r}): id {i} does not hit at its own position"
                fx, fy, t = f32(fx), f32(fy), f32(t)
                d = [f32(f32(base[k] + f32(fx * du[k])) + f32(fy * dv[k])) for k in range(3)]
                p = [f32(eye[k] + f32(t * d[k])) for k in range(3)]
                q = [f32(p[k] - lorigin[k]) for k in range(3)]
                z = dotp(q, pz)
                if not (z > 0 and z < np.inf):
                    out.outside[r, x] = True
                    continue
                gx, gy = f32(dotp(q, px) / z), f32(dotp(q, py) / z)
                if not (0 <= gx <= 1 and 0 <= gy <= 1):
                    out.outside[r, x] = True
                    continue
                li, lt, _ = oracle.closest_hit(el, float(gx), float(gy))
                out.z[r, x] = z
                out.li[r, x] = li
                out.lt[r, x] = f32(lt) if li >= 0 else f32(np.inf)
    for a in vars(out).values():
        a.setflags(write=False)
    return out


def mask_of(facts, ids, bias: float) -> np.ndarray:
    """The last two steps for every pixel: thr = z - b z (two roundings), lit iff li == id or lt >= thr."""
    b = f32(bias)
    with np.errstate(all="ignore"):
        thr = (facts.z - (b * facts.z).astype(f32)).astype(f32)
    lit = (facts.li == ids) | (facts.lt >= thr)
    mask = np.where(lit, LIT, SHADOWED).astype(np.uint8)
    mask[facts.outside] = OUTSIDE
    mask[~facts.surface] = NO_SURFACE
    return mask


def restate(view: str, light: str, w: int, h: int, wl: int, hl: int, offsets, ids, bias: float, row_begin: int = 0):
    """The definition, pixel by pixel: the mask of the band whose offsets and ids are given."""
    return mask_of(restate_facts(view, light, w, h, wl, hl, offsets, ids, row_begin), ids, bias)


@functools.lru_cache(maxsize=None)
def expected(name: str, bias: float) -> np.ndarray:
    """The expected whole-frame mask of a case (read-only, once per session)."""
    c = case(name)
    m = restate(c.view, c.light, W, H, c.wl, c.hl, c.offsets, c.ids, bias)
    m.setflags(write=False)
    return m


def counts(mask) -> tuple:
    return tuple(int((np.asarray(mask) == k).sum()) for k in range(4))


def assert_same_mask(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (f"{bad.size} classes differ, first at pixel {bad[0]}: {got.reshape(-1)[bad[0]]} != "
                           f"{want.reshape(-1)[bad[0]]}; counts {counts(got)} != {counts(want)}")


def same_bits(name, got, want):
    g = np.ascontiguousarray(got, f32).view(np.uint32).reshape(-1)
    w = np.ascontiguousarray(want, f32).view(np.uint32).reshape(-1)
    assert g.shape == w.shape, f"{name}: shape {np.shape(got)} != {np.shape(want)}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{name}: {bad.size} values differ, first at {bad[0]}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"


def same_bits_or_nan(name, got, want):
    """same_bits, except that where `want` holds a NaN `got` must hold a NaN of any sign and payload: a
    generated NaN's bits are the platform's, not the definition's."""
    g, w = np.ascontiguousarray(got, f32).reshape(-1), np.ascontiguousarray(want, f32).reshape(-1)
    assert g.shape == w.shape, f"{name}: shape {np.shape(got)} != {np.shape(want)}"
    nan = np.isnan(w)
    bad = np.flatnonzero(np.where(nan, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32)))
    assert bad.size == 0, (f"{name}: {bad.size} values differ, first at {bad[0]}: {g.view(np.uint32)[bad[0]]:#x} != "
                           f"{w.view(np.uint32)[bad[0]]:#x}")


def dimmed(shade_rgba, mask, dim: float) -> np.ndarray:
    """shade_rgba . where(mask == 1, 1, dim) in float32 on rgb; alpha unchanged; a class-3 pixel (the
    background) unmultiplied."""
    out = np.array(shade_rgba, f32)
    k = np.where(np.asarray(mask) == LIT, f32(1), f32(dim)).astype(f32)
    k = np.where(np.asarray(mask) == NO_SURFACE, f32(1), k)
    out[..., :3] = out[..., :3] * k[..., None]
    return out
