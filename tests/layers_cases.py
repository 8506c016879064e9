"""Shared cases of the depth-layer tests (test_layers_host.py, test_gpu_layers.py): the scenes, the
positions, the oracle's layers and the numpy restatement of the composite. Not a test module.

Expected layers (DESIGN.md section 2 "Layers") come from the oracle alone: oracle.closest_hit over
OracleScene.edges(W, H) is called again and again at a position, the winner's 12-float row being
overwritten with NaN after each answer -- a NaN row fails the exact test, and the other rows keep
their index -- until the first miss. Expected composites (section 2 "Composite") are a numpy float32
restatement over OracleScene.shade of each layer's id plane. Neither comes from the library.

Three cases, each a scene file with a random albedo per triangle and a background that is not
black, at a frame with partial last tiles (tiles are 64 x 16):
  stack  160 x 96   six parallel quads one behind the other, growing with depth, plus 200 soup
                    triangles: every hit count 0 .. 8 and more than 8 occurs
  twins  200 x 72   the stack with every triangle stored twice (ids i and i + N, same vertices):
                    layers k, k + 1 with equal t bits and ascending ids; hit counts are even
  q      200 x 72   query_cases' scene Q: behind-the-eye, degenerate and two frame-covering
                    (large-list) triangles; a small soup, so hit counts 0 .. 3 and more
Each case's input conditions are asserted from the oracle's answers (assert_conditions).
"""
from __future__ import annotations

import functools

import numpy as np

import query_cases as qc
from oracle import srt_oracle as oracle
from scenefile import read_scene, write_custom_scene

BACKGROUND = (0.1, 0.2, 0.3)
SHADE_TOL = 1e-5  # the project's shading tolerance against the oracle
MAX_LAYERS = 8
PEEL = MAX_LAYERS + 1  # the oracle peels one layer more: "more than 8 hits" is then visible
N_QUADS, N_SOUP = 6, 200
FRAMES = {"stack": (160, 96), "twins": (200, 72), "q": (200, 72)}
BANDS = {"stack": (21, 50), "twins": (17, 41), "q": (7, 60)}  # (row_begin, row_count): short of the frame


def stack_vertices() -> np.ndarray:
    """(12 + 200, 3, 3): quad i (two triangles, ids 2 i and 2 i + 1) at z = 3 + 0.3 i with half-size
    0.3 + 0.25 i, so the nearer quads cover less; then the soup."""
    quads = []
    for i in range(N_QUADS):
        z, h = 3.0 + 0.3 * i, 0.3 + 0.25 * i
        a, b, c, d = (-h, -h, z), (h, -h, z), (h, h, z), (-h, h, z)
        quads += [[a, b, c], [a, c, d]]
    rng = np.random.default_rng(31)
    centre = rng.uniform([-1.6, -1.2, 2.0], [1.6, 1.2, 4.5], (N_SOUP, 3))
    soup = centre[:, None, :] + rng.uniform(-0.55, 0.55, (N_SOUP, 3, 3))
    return np.concatenate([np.array(quads, np.float64), soup]).astype(np.float32)


def write_case(name: str, path) -> str:
    if name == "q":
        cam, _, v, _ = read_scene(qc.write_scene_q(str(path) + ".q"))
        kw = dict(eye=cam[0:3], lookat=cam[3:6], up=cam[6:9], vfov=cam[9])
    else:
        v = stack_vertices().reshape(-1, 9)
        if name == "twins":
            v = np.concatenate([v, v])
        kw = {}
    albedo = np.random.default_rng(41).uniform(0.2, 1.0, (len(v), 3)).astype(np.float32)
    return write_custom_scene(path, v, albedo=albedo, background=BACKGROUND, **kw)


def opacity(n: int) -> np.ndarray:
    return np.random.default_rng(43).uniform(0.1, 0.9, n).astype(np.float32)


def offsets(width: int, height: int) -> np.ndarray:
    return qc.random_offsets(width, height, 3)


def pixel_positions(width: int, height: int, off: np.ndarray) -> np.ndarray:
    """(H * W, 2) float32, row-major, from oracle.pixel_position."""
    pos = np.empty((height, width, 2), np.float32)
    for y in range(height):
        for x in range(width):
            pos[y, x] = oracle.pixel_position(x, y, float(off[y, x, 0]), float(off[y, x, 1]), width, height)
    return pos.reshape(-1, 2)


def oracle_layers(path: str, width: int, height: int, pos: np.ndarray, layers: int = PEEL):
    """(ids (layers, count) int32, t (layers, count) float32): the oracle's closest hit peeled
    `layers` times at every position; a missing layer is (-1, +inf)."""
    edges = oracle.OracleScene(path).edges(width, height).copy()
    keep = edges.copy()
    ids = np.full((layers, len(pos)), -1, np.int32)
    t = np.full((layers, len(pos)), np.inf, np.float32)
    for q, (fx, fy) in enumerate(pos):
        won = []
        for k in range(layers):
            i, tt, _ = oracle.closest_hit(edges, fx, fy)
            if i < 0:
                break
            ids[k, q], t[k, q] = i, tt
            won.append(i)
            edges[i] = np.nan
        edges[won] = keep[won]
    return ids, t


@functools.lru_cache(maxsize=None)
def cached_layers(path: str, name: str, key: str):
    """The oracle's PEEL layers for a named position set of a case, once per session, read-only.
    key: 'pixels' (the frame's pixels under offsets()) or 'mixed' (query_cases.mixed_positions).
    Returns (pos, ids, t)."""
    w, h = FRAMES[name]
    pos = pixel_positions(w, h, offsets(w, h)) if key == "pixels" else qc.mixed_positions(w, h)
    ids, t = oracle_layers(path, w, h, pos)
    for a in (pos, ids, t):
        a.setflags(write=False)
    return pos, ids, t


def assert_conditions(name: str, ids: np.ndarray, t: np.ndarray):
    """The oracle's layers (PEEL, count) hold what the case is there for."""
    hits = (ids >= 0).sum(axis=0)
    assert np.all((ids >= 0) == np.isfinite(t)) and np.all(t[ids < 0] == np.inf)
    # front to back: keys ascend strictly
    both = ids[1:] >= 0
    assert np.all((t[:-1] < t[1:])[both] | ((t[:-1] == t[1:]) & (ids[:-1] < ids[1:]))[both])
    if name == "stack":
        for c in range(MAX_LAYERS + 1):
            assert (hits == c).any(), f"no position with {c} hits"
        assert (hits > MAX_LAYERS).any()
    elif name == "twins":
        # every triangle twice: hits come in pairs, (t, i) then (t, i + N)
        n = 2 * N_QUADS + N_SOUP
        for c in (0, 2, 4, 6, 8):
            assert (hits == c).any(), f"no position with {c} hits"
        assert (hits > MAX_LAYERS).any()
        tb = t.view(np.uint32)
        equal = both & (tb[:-1] == tb[1:])
        assert equal.sum() >= 1000 and np.all((ids[1:] - ids[:-1])[equal] > 0)
        assert ((ids[1:] - ids[:-1])[equal] == n).sum() >= 1000
    else:
        for c in range(4):
            assert (hits == c).any(), f"no position with {c} hits"
        assert (hits > 3).any()
        large = np.isin(ids, qc.LARGE_IDS)
        listed = (ids >= 0) & ~large
        mixed = large.any(axis=0) & listed.any(axis=0)
        assert mixed.sum() >= 0.01 * ids.shape[1], "no position whose layers mix tile-list and large-list ids"
        # and in both orders: a covering triangle in front of and behind soup triangles
        assert (large[0] & mixed).any() or (large[1:] & listed[:-1]).any()


def assert_same(got_ids, got_t, want_ids, want_t):
    """Exact: ids equal, t equal on the uint32 view (any shape)."""
    qc.assert_same(np.asarray(got_ids).ravel(), np.asarray(got_t).ravel(), np.asarray(want_ids).ravel(),
                   np.asarray(want_t).ravel())


def shaded_layers(path: str, width: int, height: int, ids: np.ndarray, off: np.ndarray) -> np.ndarray:
    """(K, H, W, 4): OracleScene.shade of every layer's id plane (ids (K, H, W))."""
    scene = oracle.OracleScene(path)
    return np.stack([scene.shade(width, height, ids[k], off) for k in range(ids.shape[0])])


def expected_composite(shaded: np.ndarray, ids: np.ndarray, opa: np.ndarray, background) -> np.ndarray:
    """DESIGN.md section 2 "Composite" restated in numpy float32, one rounding per operation:
    shaded (K, rows, W, 4) the layers' shades, ids (K, rows, W), opa (n,) -> (rows, W, 4)."""
    n = len(opa)
    bg = np.asarray(background, np.float32)
    T = np.ones(ids.shape[1:], np.float32)
    acc = np.zeros(ids.shape[1:] + (3,), np.float32)
    live = np.ones(ids.shape[1:], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(ids.shape[0]):
            live &= (ids[k] >= 0) & (ids[k] < n)
            a = opa[np.where(live, ids[k], 0)] if n else np.zeros(ids.shape[1:], np.float32)
            w = T * a
            assert w.dtype == np.float32
            acc = np.where(live[..., None], acc + w[..., None] * shaded[k, ..., :3].astype(np.float32), acc)
            T = np.where(live, T - w, T)
        out = np.empty(ids.shape[1:] + (4,), np.float32)
        out[..., :3] = acc + T[..., None] * bg
        out[..., 3] = np.float32(1) - T
    return out


def same_bits(what: str, got: np.ndarray, want: np.ndarray):
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}: "
                           f"{np.asarray(got)[tuple(bad[0])]!r} != {np.asarray(want)[tuple(bad[0])]!r}")
