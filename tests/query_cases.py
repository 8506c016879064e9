"""Shared cases of the point-query tests (test_query_host.py, test_gpu_query.py): the test scene Q,
the position families and the oracle's answers. Not a test module."""
from __future__ import annotations

import functools

import numpy as np

from oracle import srt_oracle as oracle
from scenefile import write_custom_scene

W, H = 200, 150  # 4 x 10 tiles of 64 x 16, the last column and row partial
N_SOUP = 400     # ids [0, 400): the soup; [400, 420): behind the eye; 420, 421: degenerate; 422, 423: covering
LARGE_IDS = (422, 423)
OUT_OF_RANGE = np.array([-3.25, np.nextafter(np.float32(1), np.float32(2)), 4.5, 1e30, np.inf, -np.inf, np.nan],
                        np.float32)


def scene_q_vertices(rng):
    """Scene Q's geometry, (N_SOUP + 24, 3, 3) float32, drawn from rng (default_rng(11) for Q itself;
    scale_cases' scene S goes on drawing its albedo from the same generator)."""
    c = rng.uniform([-1.2, -0.9, 2.0], [1.2, 0.9, 4.0], (N_SOUP, 3))
    soup = c[:, None, :] + rng.uniform(-0.15, 0.15, (N_SOUP, 3, 3))
    behind = rng.uniform([-1, -1, -6], [1, 1, -0.5], (20, 3, 3))
    point = np.array([[[0.3, 0.2, 4.0]] * 3])
    line = np.array([[[0, 0, 4], [0.2, 0.2, 4], [0.4, 0.4, 4]]], np.float64)
    cover = np.array([[[-40, -40, 9 + i], [-0.05 * i, -40, 9 + i], [-0.05 * i, 40, 9 + i]] for i in range(2)], np.float64)
    v = np.concatenate([soup, behind, point, line, cover]).astype(np.float32)
    assert v.shape == (N_SOUP + 24, 3, 3)
    return v


def write_scene_q(path):
    """Scene Q: a soup in view, triangles behind the eye, a point and a collinear triangle, and two
    frame-covering triangles (the large list)."""
    return write_custom_scene(path, scene_q_vertices(np.random.default_rng(11)).reshape(-1, 9))


def boundary_values(extent: int, step: int) -> np.ndarray:
    """fl(k step / extent) for every tile boundary k, each with its float32 neighbours."""
    n = (extent + step - 1) // step
    b = (np.arange(n + 1, dtype=np.float32) * np.float32(step)) / np.float32(extent)
    return np.concatenate([b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))])


def boundary_positions(width: int, height: int, rng) -> np.ndarray:
    """Exactly 0 and 1, and k 64 / W and k 16 / H with nextafter in both directions: every boundary x
    with every boundary y, and each with random partners. Values past 1 (the partial last tile's far
    bound) and below 0 are among them: out of range, legal."""
    xs = np.concatenate([boundary_values(width, 64), np.float32([0.0, 1.0])])
    ys = np.concatenate([boundary_values(height, 16), np.float32([0.0, 1.0])])
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    rx = np.stack([xs, rng.random(xs.size, dtype=np.float32)], axis=1)
    ry = np.stack([rng.random(ys.size, dtype=np.float32), ys], axis=1)
    return np.concatenate([grid, rx, ry]).astype(np.float32)


def out_of_range_positions(rng) -> np.ndarray:
    """Each out-of-range value as x with an in-range y, as y with an in-range x, and every pair of them."""
    o = OUT_OF_RANGE
    a = np.stack([o, rng.random(o.size, dtype=np.float32)], axis=1)
    b = np.stack([rng.random(o.size, dtype=np.float32), o], axis=1)
    gx, gy = np.meshgrid(o, o, indexing="ij")
    return np.concatenate([a, b, np.stack([gx.ravel(), gy.ravel()], axis=1)]).astype(np.float32)


def in_range(pos: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (pos[:, 0] >= 0) & (pos[:, 0] <= 1) & (pos[:, 1] >= 0) & (pos[:, 1] <= 1)


def random_offsets(width: int, height: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((height, width, 2), dtype=np.float32)


def mixed_positions(width: int, height: int, seed: int = 5) -> np.ndarray:
    """2 000 random positions in [0, 1]^2, the boundary families and the out-of-range values."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.random((2000, 2), dtype=np.float32), boundary_positions(width, height, rng),
                           out_of_range_positions(rng)])


def oracle_answers(path: str, width: int, height: int, pos: np.ndarray):
    """oracle.closest_hit over the oracle's edge records: (ids int32, t float32), a miss as (-1, +inf)."""
    edges = oracle.OracleScene(path).edges(width, height)
    ids = np.empty(len(pos), np.int32)
    t = np.empty(len(pos), np.float32)
    for k, (fx, fy) in enumerate(pos):
        i, tt, _ = oracle.closest_hit(edges, fx, fy)
        ids[k] = i
        t[k] = tt if i >= 0 else np.inf
    return ids, t


def assert_mix(ids: np.ndarray, large_ids=LARGE_IDS):
    """The oracle's answers cover the cases a test relies on: hits, misses, large-list winners."""
    n = len(ids)
    assert (ids >= 0).sum() >= 0.10 * n and (ids < 0).sum() >= 0.10 * n
    assert np.isin(ids, large_ids).sum() >= 0.01 * n


def assert_same(got_ids, got_t, want_ids, want_t):
    """Exact: ids equal, t equal on the uint32 view."""
    got_ids, want_ids = np.asarray(got_ids), np.asarray(want_ids)
    bad = np.flatnonzero(got_ids != want_ids)
    assert bad.size == 0, f"{bad.size} ids differ, first at {bad[0]}: {got_ids[bad[0]]} != {want_ids[bad[0]]}"
    gt, wt = np.asarray(got_t, np.float32).view(np.uint32), np.asarray(want_t, np.float32).view(np.uint32)
    bad = np.flatnonzero(gt != wt)
    assert bad.size == 0, f"{bad.size} t differ, first at {bad[0]}: {gt[bad[0]]:#x} != {wt[bad[0]]:#x}"


@functools.lru_cache(maxsize=None)
def cached_answers(path: str, width: int, height: int, key: str):
    """The oracle's answers for a named position set of a scene, computed once per session and shared
    (read-only) by the tests that need them. key: 'pixels' (random offsets, seed 3) or 'mixed'."""
    if key == "pixels":
        import simpleraytracer_amd.device as device

        pos = device.pixel_positions(width, height, random_offsets(width, height, 3))
    else:
        pos = mixed_positions(width, height)
    ids, t = oracle_answers(path, width, height, pos)
    for a in (pos, ids, t):
        a.setflags(write=False)
    return pos, ids, t
