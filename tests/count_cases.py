"""Shared cases of the triangle-count tests (test_count_host.py, test_gpu_count.py): scenes whose
triangle count n lies on or next to a boundary of the library's own blocking -- 8 (kBvhWidth: a
partial last leaf, a partial last node, the level count), 256 (kTileTriangles, kBinThreads: the last
record block, block extent and shading-table block), 4 096 (kPadTriangles, the cull step, the minimum
list capacity) and 65 536 / 131 072 (the bit planes of the packed ids) -- and the oracle's answers.
Not a test module.

The library indexes its records by spatial-order position, not by id, so scene N(n) is built around
the order: n small triangles on a jittered grid over the inner 96 % of a 256 x 144 view at depths 4
to 6 (nothing behind the eye: no key is the last key), the ids shuffled. The order of this geometry
is computed with the float64 restatement of MortonKey (test_gpu_parity.morton_order_numpy), and the
triangles at the order positions {0, 1, 7, 8, 255, 256, n - 257, n - 256, n - 9, n - 8, n - 2, n - 1}
(sentinel_positions: the first and last record of a leaf, of a 256-record block and of the order)
and ids 0 and n - 1 are replaced by sentinels: long thin wedges with the same centroid direction
(the key, and so the position, does not move), each along its own line, so that wedges whose centres
nearly coincide (neighbours in Morton order at large n) cross only at the centre, the tip on the side
of the frame's middle (the order's ends lie in the frame's corners), and each pulled towards the eye
by its own factor: in front of the grid, at distinct depths.
A dropped last record, a pad record read as real or a last leaf left out of its parent's box then
changes pixels of the frame.

N(n, dead=d) appends d triangles behind the eye (ids n - d .. n - 1): they take key 0xFFFFFFFF, so
the order's tail -- the last leaf and, for d = 1, a whole record block -- holds only disabled
records; the live tail before them carries the sentinels.

Every case's conditions are asserted on the oracle's answers here (guards), so no test of a case
passes vacuously. Files and answers are made once per session and shared read-only.
"""
from __future__ import annotations

import atexit
import functools
import math
import shutil
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import layers_cases as lc
import query_cases as qc
from oracle import srt_oracle as oracle
from scenefile import write_custom_scene
from test_gpu_parity import morton_order_numpy

f32 = np.float32
SMALL = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193)
LARGE = (32767, 32768, 32769, 65535, 65536, 65537, 131071, 131072)
DEAD = ((9, 1), (16, 8), (257, 1), (264, 8), (4097, 1), (4104, 9))  # (n, the last d ids behind the eye)
PLANE_COUNTS = (65535, 65536, 65537, 131071, 131072)
W, H = 256, 144        # 4 x 9 tiles of 64 x 16, all full; the scenes are built for this frame
ODD_W, ODD_H = 200, 72  # a last tile column of 8 pixels, a last tile row of 8 rows
BACKGROUND = (0.1, 0.2, 0.3)
VFOV = 60.0
LAYERS = 4
WEDGE_L, WEDGE_W = 30.0, 3.0  # pixels: the tip at c + L d, the base at c - L / 2 d +- w n
HALF_H = math.tan(VFOV * math.pi / 360.0)
HALF_W = HALF_H * W / H


def name_of(n: int, dead: int = 0) -> str:
    return f"n{n}d{dead}" if dead else f"n{n}"


SMALL_NAMES = tuple(name_of(n) for n in SMALL)
LARGE_NAMES = tuple(name_of(n) for n in LARGE)
DEAD_NAMES = tuple(name_of(n, d) for n, d in DEAD)
ALL_NAMES = SMALL_NAMES + LARGE_NAMES + DEAD_NAMES


def parse(name: str):
    n, _, d = name[1:].partition("d")
    return int(n), int(d or 0)


def sentinel_positions(live: int, n: int):
    """The order positions that carry sentinels: the edges of the first two leaves and record blocks
    and of the last ones, counted from the end of the order (n) and of its live part."""
    at = {0, 1, 7, 8, 255, 256}
    for m in (live, n):
        at |= {m - 257, m - 256, m - 9, m - 8, m - 2, m - 1}
    return sorted(p for p in at if 0 <= p < live)


@functools.lru_cache(maxsize=None)
def _dir() -> Path:
    d = tempfile.mkdtemp(prefix="count_cases_")
    atexit.register(shutil.rmtree, d, True)
    return Path(d)


def world(px, py, z):
    """The point at depth z that the 256 x 144 frame sees at pixel position (px, py): the camera is
    at the origin, looks along +z with +y up; the ray of (px, py) is base + px / W du + py / H dv."""
    px, py, z = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(z, np.float64))
    return np.stack([z * HALF_W * (1.0 - 2.0 * px / W), z * HALF_H * (1.0 - 2.0 * py / H), z], axis=-1)


def screen(p):
    """Pixel position (px, py) of world points (..., 3): world()'s inverse."""
    p = np.asarray(p, np.float64)
    return np.stack([(1.0 - p[..., 0] / p[..., 2] / HALF_W) * W / 2.0, (1.0 - p[..., 1] / p[..., 2] / HALF_H) * H / 2.0],
                    axis=-1)


def grid_vertices(live: int, rng) -> np.ndarray:
    """(live, 3, 3) float32: one triangle per cell of a jittered grid over the inner 96 % of the view,
    a quarter of the cell's area, each at one depth in [4, 6]; the ids are shuffled."""
    cols = max(1, math.ceil(math.sqrt(live * W / H)))
    rows = math.ceil(live / cols)
    cells = rng.permutation(cols * rows)[:live]
    cw, ch = 0.96 * W / cols, 0.96 * H / rows
    cx = 0.02 * W + (cells % cols + 0.5 + rng.uniform(-0.3, 0.3, live)) * cw
    cy = 0.02 * H + (cells // cols + 0.5 + rng.uniform(-0.3, 0.3, live)) * ch
    radius = 0.45 * min(cw, ch)
    angle = rng.uniform(0, 2 * np.pi, live)[:, None] + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.3, 0.3, (live, 3))
    z = rng.uniform(4.0, 6.0, live)[:, None]
    return world(cx[:, None] + radius * np.cos(angle), cy[:, None] + radius * np.sin(angle), z).astype(f32)


def wedge(v, k: int, m: int) -> np.ndarray:
    """The k-th of m sentinels in place of triangle v (3, 3): a wedge through v's centroid direction,
    along the line at angle pi k / m."""
    c3 = np.asarray(v, np.float64).mean(axis=0)
    c = screen(c3)
    a = np.pi * k / m
    d, nrm = np.array([np.cos(a), np.sin(a)]), np.array([-np.sin(a), np.cos(a)])
    if d @ (np.array([W / 2, H / 2]) - c) < 0:
        d = -d  # the tip towards the middle of the frame: the tails lie in its corners
    pts = np.stack([c + WEDGE_L * d, c - WEDGE_L / 2 * d + WEDGE_W * nrm, c - WEDGE_L / 2 * d - WEDGE_W * nrm])
    return world(pts[:, 0], pts[:, 1], c3[2] * (0.2 + 0.02 * k)).astype(f32)


def _write(path, v, albedo):
    return write_custom_scene(path, v.reshape(-1, 9), albedo, eye=(0, 0, 0), lookat=(0, 0, 1), up=(0, 1, 0), vfov=VFOV,
                              background=BACKGROUND)


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    """Scene N(n, dead): (name, path, n, live, dead, order, positions, sentinels, centroids) -- the
    restated spatial order, the sentinels' order positions, their ids (those at the positions, then ids
    0 and live - 1 if not among them) and their centroids as image positions of the 256 x 144 frame."""
    n, dead = parse(name)
    live = n - dead
    assert live >= 1
    rng = np.random.default_rng(1000 * n + dead)
    v = grid_vertices(live, rng)
    if dead:
        centre = rng.uniform([-1, -1, -6], [1, 1, -4], (dead, 3))
        v = np.concatenate([v, (centre[:, None, :] + rng.uniform(-0.2, 0.2, (dead, 3, 3))).astype(f32)])
    albedo = rng.uniform(0.2, 1.0, (n, 3)).astype(f32)
    path = _dir() / f"{name}.srt"
    positions = sentinel_positions(live, n)
    before = morton_order_numpy(_write(path, v, albedo))
    sentinels = [int(i) for i in before[positions]]
    sentinels += [i for i in (0, live - 1) if i not in sentinels]
    for k, i in enumerate(sentinels):
        v[i] = wedge(v[i], k, len(sentinels))
    order = morton_order_numpy(_write(path, v, albedo))
    # the replacement moved no key: the sentinels sit where the tails are
    assert np.array_equal(order[positions], before[positions]), f"{name}: a sentinel left its order position"
    if dead:
        assert np.array_equal(np.sort(order[live:]), np.arange(live, n)), f"{name}: the dead ids are not the order's tail"
    centroids = screen(v[sentinels].astype(np.float64).mean(axis=1)) / np.array([W, H])
    assert np.all((centroids > 0.01) & (centroids < 0.99))
    for a in (order, centroids):
        a.setflags(write=False)
    return SimpleNamespace(name=name, path=str(path), n=n, live=live, dead=dead, order=order, positions=tuple(positions),
                           sentinels=tuple(sentinels), centroids=centroids)


def offsets(w: int, h: int, kind: str = "rnd"):
    """A frame's sample offsets by kind: 'rnd' and 'rnd2' random, 'half' uniform 0.5 (None)."""
    if kind == "half":
        return None
    return np.random.default_rng({"rnd": 3, "rnd2": 4}[kind]).random((h, w, 2), f32)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, f32).view(np.uint32)


def frame(name: str, kind: str = "rnd", w: int = W, h: int = H) -> np.ndarray:
    """The oracle's frame of a case under offsets(w, h, kind). The case's guards are asserted on the
    'rnd' frame at 256 x 144."""
    return _frame(name, kind, w, h)


@functools.lru_cache(maxsize=None)
def _frame(name, kind, w, h):
    c = case(name)
    sc = oracle.OracleScene(c.path)
    out = sc.render(w, h, offsets(w, h, kind))
    sc.close()
    out.setflags(write=False)
    if kind == "rnd" and (w, h) == (W, H):
        _guard_frame(c, out)
    return out


def _guard_frame(c, fr):
    ids = fr[..., 3]
    won = np.unique(ids[ids >= 0]).astype(np.int64)
    lost = sorted(set(c.sentinels) - set(won.tolist()))
    assert not lost, f"{c.name}: sentinels {lost} win no pixel of the oracle's frame"
    assert 0 in won and c.live - 1 in won
    hit = float((ids >= 0).mean())
    if c.n >= 7:
        assert 0.03 <= hit <= 0.6, (c.name, hit)
    assert (ids < 0).any()
    assert not (won >= c.live).any(), f"{c.name}: a triangle behind the eye wins a pixel"


def frame_ids(name: str) -> np.ndarray:
    fr = frame(name)
    ids = fr[..., 3].astype(np.int32)
    assert np.array_equal(ids.astype(f32), fr[..., 3])
    return ids


@functools.lru_cache(maxsize=None)
def sentinel_points(name: str) -> np.ndarray:
    """(2 m, 2) float32: each sentinel's centroid, and the position of one pixel of the oracle's
    256 x 144 'rnd' frame that it wins."""
    c = case(name)
    ids = frame_ids(name)
    off = offsets(W, H)
    won = []
    for i in c.sentinels:
        y, x = np.argwhere(ids == i)[0]
        won.append(oracle.pixel_position(int(x), int(y), float(off[y, x, 0]), float(off[y, x, 1]), W, H))
    out = np.concatenate([c.centroids.astype(f32), np.array(won, f32)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def answers(name: str):
    """(pos, ids, t): the oracle's closest hit at query_cases.mixed_positions of the 256 x 144 frame
    followed by sentinel_points(). Every sentinel is the answer somewhere."""
    c = case(name)
    pos = np.concatenate([qc.mixed_positions(W, H), sentinel_points(name)])
    ids, t = qc.oracle_answers(c.path, W, H, pos)
    for a in (pos, ids, t):
        a.setflags(write=False)
    lost = sorted(set(c.sentinels) - set(ids.tolist()))
    assert not lost, f"{name}: sentinels {lost} answer at no position"
    assert (ids < 0).sum() >= 0.05 * len(ids)
    if c.n >= 7:
        assert (ids >= 0).sum() >= 0.03 * len(ids)
    return pos, ids, t


@functools.lru_cache(maxsize=None)
def layers(name: str):
    """(pos, ids (4, count), t (4, count)): layers_cases' peel of the oracle's closest hit, K = 4, at
    answers()' positions; layer 0 is answers()'."""
    c = case(name)
    pos, ids0, t0 = answers(name)
    ids, t = lc.oracle_layers(c.path, W, H, pos, LAYERS)
    for a in (ids, t):
        a.setflags(write=False)
    lc.assert_same(ids[0], t[0], ids0, t0)
    if c.n >= 63:
        assert (ids[1] >= 0).any(), f"{name}: no position with two hits"
    return pos, ids, t


@functools.lru_cache(maxsize=None)
def odd_layers(name: str):
    """(ids, t) (4, 72, 200): the peel at the pixels of the 200 x 72 frame under offsets()."""
    c = case(name)
    pos = lc.pixel_positions(ODD_W, ODD_H, offsets(ODD_W, ODD_H))
    ids, t = lc.oracle_layers(c.path, ODD_W, ODD_H, pos, LAYERS)
    assert np.array_equal(ids[0].reshape(ODD_H, ODD_W).astype(f32), frame(name, "rnd", ODD_W, ODD_H)[..., 3])
    ids, t = ids.reshape(LAYERS, ODD_H, ODD_W), t.reshape(LAYERS, ODD_H, ODD_W)
    for a in (ids, t):
        a.setflags(write=False)
    return ids, t


# The shadow families (test_gpu_count.test_shadow_families): two spot lights beside the view's eye,
# looking at the middle of the grid, and a point light at the first one's eye.
L1 = (0.6, 0.0, 0.0, 0.0, 0.0, 5.0, 0.0, 1.0, 0.0, 70.0)
L2 = (0.0, 0.6, 0.0, 0.0, 0.0, 5.0, 0.0, 1.0, 0.0, 70.0)
LIGHT_CAMS = {"L1": L1, "L2": L2}
POINT_ORIGIN = L1[:3]
FACE_SIZE = 64
SHADOW_DIM = 0.25
LIGHT_COLORS = ((1.0, 0.9, 0.8), (0.2, 0.3, 0.9), (0.6, 0.8, 0.4))  # L1, L2, the point light
LIGHT_FALLOFF = (0.0, 0.0, 9.0)
AMBIENT = (0.05, 0.04, 0.03)
SHADOW_NAMES = ("n9", "n255", "n256", "n257", "n4095", "n4096", "n4097", "n257d1", "n4097d1")
# The light under which the last live record of the *light's* order decides a pixel of the mask
# (guard (b) of shadow_answers). n9 and n257 have none: no light position tried (sixteen eyes around
# the view's) puts that record between the light and another triangle's visible pixel, so those two
# cases run without the guard.
KNOCK_OUT = {"n255": "L2", "n256": "L1", "n4095": "L1", "n4096": "L1", "n4097": "L2", "n257d1": "L1", "n4097d1": "L1"}


def host_lights():
    from simpleraytracer_amd import PointLightHost, SpotLightHost

    return [SpotLightHost(L1, W, H, LIGHT_COLORS[0], LIGHT_FALLOFF[0], 0.0),
            SpotLightHost(L2, W, H, LIGHT_COLORS[1], LIGHT_FALLOFF[1], 0.0),
            PointLightHost(POINT_ORIGIN, FACE_SIZE, LIGHT_COLORS[2], LIGHT_FALLOFF[2], 0.0)]


@functools.lru_cache(maxsize=None)
def shadow_answers(name: str) -> SimpleNamespace:
    """The host paths' answers for the whole 256 x 144 frame under offsets() and frame_ids(): spot
    (mask, rgba) under L1 at SHADOW_DIM, omni (mask, face, rgba) under the point light, lighting (rgba,
    classes) under host_lights() and AMBIENT. Guards: (a) L1's mask holds at least 100 shadowed (n9: 9)
    and 100 lit pixels; (b) for the cases of KNOCK_OUT, moving the last live record of the light's order
    behind both eyes changes the mask at a pixel of another triangle -- a walk that drops the last
    record of a list or of the stream answers wrongly there."""
    from simpleraytracer_amd import device

    c = case(name)
    off, ids = offsets(W, H), frame_ids(name)
    spot = device.shadow_host(c.path, W, H, L1, W, H, off, ids, dim=SHADOW_DIM)
    omni = device.omni_shadow_host(c.path, W, H, POINT_ORIGIN, FACE_SIZE, off, ids, dim=SHADOW_DIM)
    lighting = device.lighting_host(c.path, W, H, host_lights(), AMBIENT, off, ids)
    counts = np.bincount(spot[0].ravel(), minlength=4)
    # (n9's nine triangles shadow 9 pixels of one another under L1; every other case at least 277)
    assert counts[0] >= (9 if name == "n9" else 100) and counts[1] >= 100, f"{name}: classes {counts.tolist()} of L1's mask"
    assert np.array_equal(lighting[1][0], spot[0]) and np.array_equal(lighting[1][2], omni[0])
    if name in KNOCK_OUT:
        cam = LIGHT_CAMS[KNOCK_OUT[name]]
        sc = device.read_scene(c.path)
        v = sc["vertices"].copy()
        j = int(device.order_host(v, cam)[0][c.live - 1])
        v[j] = (0.0, 0.0, -5.0, 0.1, 0.0, -5.0, 0.0, 0.1, -5.0)  # behind the view's eye and the light's
        without = _write(_dir() / f"{name}_without_{j}.srt", v, sc["albedo"])
        full = spot[0] if cam is L1 else device.shadow_host(c.path, W, H, cam, W, H, off, ids)[0]
        mask = device.shadow_host(without, W, H, cam, W, H, off, ids)[0]
        assert ((mask != full) & (ids != j)).any(), f"{name}: the light order's last record {j} decides no pixel"
    for a in (*spot, *omni, *lighting):
        a.setflags(write=False)
    return SimpleNamespace(spot=spot, omni=omni, lighting=lighting)


def id_planes(n: int) -> int:
    """The bit planes above 16 that the packed hit ids of n triangles need: the codes are 0 .. n - 1
    and the miss code is all ones, so they fit 16 + p bits while n <= 2^(16 + p) - 1."""
    return max(0, n.bit_length() - 16)


def packed_band_bytes(planes: int, rows: int, width: int) -> int:
    """A band's packed ids: per row 2 B a pixel (rounded up to 8 B) plus 8 B per plane and 64 pixels,
    per 16-row tile row one 8-B offset per 64-pixel tile, padded to 256 B."""
    words = (width + 63) // 64
    row = (width * 2 + 7) // 8 * 8 + planes * words * 8
    return ((rows + 15) // 16 * (16 * row + words * 8) + 255) // 256 * 256
