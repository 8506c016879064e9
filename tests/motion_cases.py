"""Shared cases of the motion tests (test_motion_host.py, test_gpu_motion.py; include/srt_motion.h):
hand-built scenes at two camera poses and two vertex poses, and the oracle's answers for every
combination -- never the library's. Not a test module.

Scene M(n), n in COUNTS = 1, 257, 4097 (one triangle; one past a leaf / record block; one past
kPadTriangles -- where the sort, the gather and the pad records can each go wrong): n triangles
scattered through a box around (0, 0, 5), sized so that they cover about half of camera A's frame.
  camera A   eye (0, 0, 0), towards +z, up +y, vfov 60;
  camera B   another eye, direction, up and vfov: the image-plane Morton order really changes;
  V0         the mesh as built;
  V1         V0 turned by 70 degrees about an axis through the box's centre plus a displacement of
             every vertex, and (n > 1) its last max(1, n / 16) triangles carried behind both eyes:
             their key becomes the last key, so the order's tail changes too.
A file exists per (n, vertex pose, camera); the albedo and the background are the same in all of
them, as an update leaves them.

Guards (check(n), on the oracle's frames and the float64 restatement of the key alone, so that no
test passes vacuously): between A and B and between V0 and V1 at least a quarter of the pixels
change id; the order changes in more than half of its positions (n > 1: a one-entry order has one
value); every frame has hits and misses. One triangle cannot both be seen and lie behind the eye, so
M(1)'s V1 only turns and shifts it.
"""
from __future__ import annotations

import atexit
import functools
import shutil
import tempfile
from pathlib import Path

import numpy as np

from oracle import srt_oracle as oracle
from scenefile import write_custom_scene
from test_gpu_parity import morton_order_numpy

f32 = np.float32
COUNTS = (1, 257, 4097)
W, H = 256, 144          # 4 x 9 full tiles
ODD_W, ODD_H = 200, 72   # a last tile column of 8 pixels, a last tile row of 8 rows (count_cases.ODD_*)
SIZES = ((W, H), (ODD_W, ODD_H))
LIGHT = 64               # light frames: 64 x 64
BACKGROUND = (0.1, 0.2, 0.3)
CENTRE = np.array([0.0, 0.0, 5.0])
# eye, lookat, up, vfov
CAMERAS = {
    "A": (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 60.0),
    "B": (3.0, 1.5, 1.0, 1.5, -0.75, 5.0, 0.25, 1.0, 0.125, 45.0),
}
# Light poses: two spot-light cameras and two omni-light origins (all see the box).
SPOTS = {
    0: (-2.5, 3.0, 1.5, 0.0, 0.0, 5.0, 0.0, 1.0, 0.0, 70.0),
    1: (2.0, 3.5, 2.5, 0.5, -0.5, 5.5, 0.0, 0.0, 1.0, 55.0),
}
ORIGINS = {0: (0.5, 2.5, 3.0), 1: (-1.25, 1.75, 6.5)}
POSES = (("camera", 0, "A", 0, "B"), ("vertices", 0, "A", 1, "A"), ("both", 0, "A", 1, "B"))


@functools.lru_cache(maxsize=None)
def _dir() -> Path:
    d = tempfile.mkdtemp(prefix="motion_cases_")
    atexit.register(shutil.rmtree, d, True)
    return Path(d)


def _rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(degrees)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


@functools.lru_cache(maxsize=None)
def vertices(n: int, pose: int) -> np.ndarray:
    """(n, 9) float32, read-only."""
    rng = np.random.default_rng(100 + n)
    if n == 1:
        v = np.array([[[-5.0, -3.2, 5.0], [5.0, -2.0, 5.6], [0.5, 3.4, 4.4]]])
    else:
        half = np.array([3.4, 2.0, 1.0])
        c = CENTRE + rng.uniform(-half, half, (n, 3))
        r = 2.2 * np.sqrt(4 * half[0] * half[1] / n)  # about half of the box's front face covered
        v = c[:, None, :] + rng.uniform(-r, r, (n, 3, 3))
    if pose == 1:
        v = (v - CENTRE) @ _rotation((0.3, 0.4, 1.0), 70.0).T + CENTRE
        # (one triangle alone has to travel further for a quarter of the narrow frame's pixels to change)
        v = v + rng.uniform(-0.08, 0.08, v.shape) + np.array([3.5, -1.5, 0.2] if n == 1 else [0.5, -0.3, 0.2])
        if n > 1:
            dead = max(1, n // 16)
            v[n - dead:] += np.array([0.0, 0.0, -11.0])  # around (0, 0, -6): behind A's eye and B's
    out = np.ascontiguousarray(v.astype(f32).reshape(n, 9))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def albedo(n: int) -> np.ndarray:
    a = np.random.default_rng(200 + n).uniform(0.2, 1.0, (n, 3)).astype(f32)
    a.setflags(write=False)
    return a


def _write(name: str, n: int, pose: int, cam) -> str:
    path = _dir() / name
    if not path.exists():
        write_custom_scene(path, vertices(n, pose), albedo(n), eye=cam[0:3], lookat=cam[3:6], up=cam[6:9], vfov=cam[9],
                           background=BACKGROUND)
    return str(path)


def path(n: int, pose: int, cam: str) -> str:
    """The file of M(n) at vertex pose `pose` under camera `cam` ("A" / "B")."""
    return _write(f"m{n}_v{pose}_{cam}.srt", n, pose, CAMERAS[cam])


def spot_path(n: int, pose: int, k: int) -> str:
    """The same triangles under spot-light camera SPOTS[k]."""
    return _write(f"m{n}_v{pose}_spot{k}.srt", n, pose, SPOTS[k])


@functools.lru_cache(maxsize=None)
def offsets(w: int, h: int, j: int = 0) -> np.ndarray:
    """Sample offsets (h, w, 2) of a w x h frame; j: the j-th set (batches, sample planes)."""
    out = np.random.default_rng(7 * w + h + 1000 * j).random((h, w, 2), f32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frame(n: int, pose: int, cam: str, w: int = W, h: int = H, j: int = 0) -> np.ndarray:
    """The oracle's RGBA frame (h, w, 4) under offsets(w, h, j), alpha = the id (-1: a miss), once
    per session."""
    sc = oracle.OracleScene(path(n, pose, cam))
    out = sc.render(w, h, np.array(offsets(w, h, j)))
    sc.close()
    out.setflags(write=False)
    return out


def ids(n: int, pose: int, cam: str, w: int = W, h: int = H, j: int = 0) -> np.ndarray:
    fr = frame(n, pose, cam, w, h, j)
    out = fr[..., 3].astype(np.int32)
    assert np.array_equal(out.astype(f32), fr[..., 3])
    return out


@functools.lru_cache(maxsize=None)
def order(n: int, pose: int, cam: str) -> np.ndarray:
    """The float64 numpy restatement of the spatial order (test_gpu_parity.morton_order_numpy)."""
    out = morton_order_numpy(path(n, pose, cam))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def check(n: int) -> bool:
    """The guards of M(n); every test calls it before it trusts a comparison."""
    for w, h in SIZES:
        for pose, cam in ((0, "A"), (0, "B"), (1, "A"), (1, "B")):
            i = ids(n, pose, cam, w, h)
            assert (i >= 0).mean() >= 0.05 and (i < 0).mean() >= 0.05, (n, pose, cam, w, h, float((i >= 0).mean()))
        for (p0, c0), (p1, c1) in (((0, "A"), (0, "B")), ((0, "A"), (1, "A")), ((0, "A"), (1, "B"))):
            changed = float((ids(n, p0, c0, w, h) != ids(n, p1, c1, w, h)).mean())
            assert changed >= 0.25, (n, (p0, c0), (p1, c1), w, h, changed)
    if n > 1:
        for a, b in (((0, "A"), (0, "B")), ((0, "A"), (1, "A")), ((0, "A"), (1, "B"))):
            moved = float((order(n, *a) != order(n, *b)).mean())
            assert moved > 0.5, (n, a, b, moved)
        v1 = vertices(n, 1).reshape(n, 3, 3).astype(np.float64)
        dead = max(1, n // 16)
        assert (v1[n - dead:, :, 2] < 0).all()
        for cam in ("A", "B"):  # behind the eye: the last key, so the order's tail is the dead ids
            assert np.array_equal(np.sort(order(n, 1, cam)[n - dead:]), np.arange(n - dead, n)), (n, cam)
            won = np.unique(ids(n, 1, cam))
            assert not (won >= n - dead).any()
    return True


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, f32).view(np.uint32)
