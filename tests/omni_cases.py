"""Shared cases of the omni-light shadow tests (test_omni_host.py, test_gpu_omni.py): the room
scene, the numpy float32 restatement of DESIGN.md section 2 "Omni shadow" and the expected masks and
face planes -- from the oracle and numpy, never from the library. Not a test module.

The restatement is shadow_cases.restate's loop with the face choice inserted between its steps 5
and 6; the six face frames come from six files written with the table's cameras
(OracleScene(face file).edges(F, F) / .frame(F, F)). A view's facts at a face size (face, depth,
the face frame's closest hit) are computed once per session and shared read-only; the mask of a
bias follows from them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import srt_oracle as oracle
from shadow_cases import (H, LIT, NO_SURFACE, OUTSIDE, SHADOWED, W, _dir, assert_same_mask, dimmed, dotp,  # noqa: F401
                          projection_rows, random_offsets, same_bits, write_with_camera)

f32 = np.float32
NO_FACE = 255
BIASES = (0.0, 2.0 ** -10)
FACE_SIZES = (64, 200)  # 200: partial last tile columns and rows
VFOV = 92.0
ORIGIN = (0.25, 1.0, 4.0)
# face -> (axis, up)
FACES = (((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, -1)),
         ((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)))
VIEWS = {
    "A": (-2.6, 2.6, 1.4, 1.5, 0.0, 6.0, 0.0, 1.0, 0.0, 75.0),
    "B": (2.6, 2.5, 6.6, -1.5, 0.0, 2.0, 0.0, 1.0, 0.0, 75.0),
}


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def room_vertices() -> np.ndarray:
    """A closed box (12 triangles), two occluder quads (4) and 200 soup triangles inside it."""
    x0, x1, y0, y1, z0, z1 = -3.0, 3.0, -1.0, 3.0, 1.0, 7.0
    box = (_quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)) +  # floor
           _quad((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)) +  # ceiling
           _quad((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)) +  # x = -3
           _quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)) +  # x = +3
           _quad((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)) +  # z = 1
           _quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)))   # z = 7
    occ_y = _quad((-0.5, 0.0, 3.5), (0.5, 0.0, 3.5), (0.5, 0.0, 4.5), (-0.5, 0.0, 4.5))
    occ_x = _quad((1.5, 0.0, 3.0), (1.5, 2.0, 3.0), (1.5, 2.0, 5.0), (1.5, 0.0, 5.0))
    rng = np.random.default_rng(7)
    c = rng.uniform([-2.5, -0.8, 1.5], [2.5, 2.8, 6.5], (200, 3))
    soup = c[:, None, :] + rng.uniform(-0.15, 0.15, (200, 3, 3))
    return np.concatenate([np.array(box), np.array(occ_y), np.array(occ_x), soup]).astype(f32).reshape(-1, 9)


def face_camera(origin, k: int) -> tuple:
    """(eye, lookat, up, vfov) of face k: lookat = fl32(o + axis)."""
    axis, up = FACES[k]
    o = [f32(v) for v in origin]
    look = [float(f32(o[j] + f32(axis[j]))) for j in range(3)]
    return tuple(float(v) for v in o) + tuple(look) + tuple(float(v) for v in up) + (VFOV,)


def face_of(q) -> int:
    """The definition's face choice on three float32 values."""
    a = [np.abs(f32(v)) for v in q]
    m = 0
    with np.errstate(invalid="ignore"):
        if a[1] > a[m]:
            m = 1
        if a[2] > a[m]:
            m = 2
        return 2 * m + (1 if f32(q[m]) < 0 else 0)


@functools.lru_cache(maxsize=None)
def case(view: str) -> SimpleNamespace:
    """The view's file, the six face files, the view frame's sample offsets and the oracle's hit ids."""
    v = room_vertices()
    path = write_with_camera(_dir() / f"omni_{view}.srt", v, VIEWS[view])
    faces = tuple(write_with_camera(_dir() / f"omni_{view}_face{k}.srt", v, face_camera(ORIGIN, k)) for k in range(6))
    off = random_offsets()
    sc = oracle.OracleScene(path)
    ids = sc.render(W, H, off)[..., 3].astype(np.int32)
    sc.close()
    for a in (off, ids):
        a.setflags(write=False)
    return SimpleNamespace(name=view, view=path, faces=faces, origin=ORIGIN, n=len(v), offsets=off, ids=ids)


def restate(c, face_size: int, offsets, ids, row_begin: int = 0, w: int = W, h: int = H) -> SimpleNamespace:
    """The definition up to the bias, pixel by pixel, for the band whose offsets and ids are given:
    face (255: no surface), outside (class 2), z, the face frame's closest hit (li, lt), the
    frustum margin min(g, 1 - g) and whether the pixel is near a cube seam. The view frame is w x h."""
    sv = oracle.OracleScene(c.view)
    n = sv.n
    ev, fv = sv.edges(w, h), sv.frame(w, h)
    sv.close()
    el, rows_f, origin_f = [], [], []
    for k in range(6):
        s = oracle.OracleScene(c.faces[k])
        assert s.n == n
        el.append(s.edges(face_size, face_size))
        fl = s.frame(face_size, face_size)
        s.close()
        rows_f.append(projection_rows(fl))
        origin_f.append(fl[0:3])
    assert all(np.array_equal(o, origin_f[0]) for o in origin_f)
    lorigin = origin_f[0]
    eye, base, du, dv = fv[0:3], fv[3:6], fv[6:9], fv[9:12]
    rows = ids.shape[0]
    out = SimpleNamespace(face=np.full((rows, w), NO_FACE, np.uint8), outside=np.zeros((rows, w), bool),
                          z=np.zeros((rows, w), f32), li=np.full((rows, w), -1, np.int64),
                          lt=np.full((rows, w), np.inf, f32), margin=np.full((rows, w), np.inf),
                          seam=np.zeros((rows, w), bool))
    with np.errstate(all="ignore"):
        for r in range(rows):
            for x in range(w):
                i = int(ids[r, x])
                if not 0 <= i < n:
                    continue
                fx, fy = oracle.pixel_position(x, row_begin + r, float(offsets[r, x, 0]), float(offsets[r, x, 1]), w, h)
                hit, t, _ = oracle.closest_hit(ev[i:i + 1], fx, fy)
                assert hit == 0, f"pixel ({x}, {row_begin + r}): id {i} does not hit at its own position"
                fx, fy, t = f32(fx), f32(fy), f32(t)
                d = [f32(f32(base[k] + f32(fx * du[k])) + f32(fy * dv[k])) for k in range(3)]
                p = [f32(eye[k] + f32(t * d[k])) for k in range(3)]
                q = [f32(p[k] - lorigin[k]) for k in range(3)]
                face = face_of(q)
                out.face[r, x] = face
                a = sorted(abs(float(v)) for v in q)
                out.seam[r, x] = a[1] >= 0.99 * a[2]
                px, py, pz = rows_f[face]
                z = dotp(q, pz)
                if not (z > 0 and z < np.inf):
                    out.outside[r, x] = True
                    continue
                gx, gy = f32(dotp(q, px) / z), f32(dotp(q, py) / z)
                if not (0 <= gx <= 1 and 0 <= gy <= 1):
                    out.outside[r, x] = True
                    continue
                out.margin[r, x] = min(float(gx), 1.0 - float(gx), float(gy), 1.0 - float(gy))
                li, lt, _ = oracle.closest_hit(el[face], float(gx), float(gy))
                out.z[r, x] = z
                out.li[r, x] = li
                out.lt[r, x] = f32(lt) if li >= 0 else f32(np.inf)
    for a in vars(out).values():
        a.setflags(write=False)
    return out


def mask_of(facts, ids, bias: float) -> np.ndarray:
    """Steps 9 and 10 for every pixel: thr = z - b z (two roundings), lit iff li == id or lt >= thr."""
    b = f32(bias)
    with np.errstate(all="ignore"):
        thr = (facts.z - (b * facts.z).astype(f32)).astype(f32)
    lit = (facts.li == ids) | (facts.lt >= thr)
    mask = np.where(lit, LIT, SHADOWED).astype(np.uint8)
    mask[facts.outside] = OUTSIDE
    mask[facts.face == NO_FACE] = NO_SURFACE
    return mask


@functools.lru_cache(maxsize=None)
def facts(view: str, face_size: int) -> SimpleNamespace:
    c = case(view)
    return restate(c, face_size, c.offsets, c.ids)


@functools.lru_cache(maxsize=None)
def expected(view: str, face_size: int, bias: float) -> np.ndarray:
    """The expected whole-frame mask (read-only, once per session); the face plane is
    facts(view, face_size).face."""
    m = mask_of(facts(view, face_size), case(view).ids, bias)
    m.setflags(write=False)
    return m


def assert_same_face(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (f"{bad.size} faces differ, first at pixel {bad[0]}: {got.reshape(-1)[bad[0]]} != "
                           f"{want.reshape(-1)[bad[0]]}")


def check_expected(view: str, face_size: int):
    """What keeps a test from hiding a failure: every face selected, both classes on every face,
    seam pixels present, no class 2, the frustum margin the 92 degree faces promise."""
    fa = facts(view, face_size)
    assert (fa.face != NO_FACE).all(), "every pixel of the room's views hits a surface"
    assert not fa.outside.any(), f"{int(fa.outside.sum())} class-2 pixels"
    assert int(fa.seam.sum()) >= 100, f"only {int(fa.seam.sum())} near-seam pixels"
    assert float(fa.margin.min()) > 0.015, f"frustum margin {float(fa.margin.min())}"
    for bias in BIASES:
        m = expected(view, face_size, bias)
        for k in range(6):
            on = fa.face == k
            assert int((m[on] == SHADOWED).sum()) >= 20 and int((m[on] == LIT).sum()) >= 20, \
                f"view {view} F {face_size} bias {bias} face {k}: {int((m[on] == SHADOWED).sum())} shadowed, " \
                f"{int((m[on] == LIT).sum())} lit"
