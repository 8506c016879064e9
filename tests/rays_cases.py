"""Shared cases of the ray-query tests (test_rays_host.py, test_gpu_rays.py): the scenes, the ray
families with fixed seeds and the host's answers. Not a test module.

A ray is 8 float32 values (ox, oy, oz, tmin, dx, dy, dz, tmax) (DESIGN.md section 2 "Rays")."""
from __future__ import annotations

import atexit
import functools
import shutil
import tempfile
from pathlib import Path

import numpy as np

import query_cases as qc
from scenefile import read_scene, write_custom_scene

f32 = np.float32
INF = f32(np.inf)
COUNT_SOUPS = (0, 1, 7, 8, 9, 63, 64, 65, 512, 513, 4097)  # where the 8-wide tree's shape changes
FINE_N, FINE_SIZE = 2000, 0.03


@functools.lru_cache(maxsize=None)
def _dir() -> Path:
    d = tempfile.mkdtemp(prefix="rays_cases_")
    atexit.register(shutil.rmtree, d, True)
    return Path(d)


def soup_vertices(n: int, seed: int, size: float = 0.15) -> np.ndarray:
    rng = np.random.default_rng(seed)
    c = rng.uniform([-1.2, -0.9, 2.0], [1.2, 0.9, 4.0], (n, 3))
    return (c[:, None, :] + rng.uniform(-size, size, (n, 3, 3))).astype(f32).reshape(n, 9)


@functools.lru_cache(maxsize=None)
def soup_path(n: int, size: float = 0.15) -> str:
    return write_custom_scene(_dir() / f"soup{n}_{size}.srt", soup_vertices(n, 100 + n, size))


@functools.lru_cache(maxsize=None)
def q_path() -> str:
    return qc.write_scene_q(_dir() / "q.srt")


@functools.lru_cache(maxsize=None)
def q_chunk_path() -> str:
    """The last 64 triangles of scene Q: 40 of the soup, the 20 behind the origin, the point, the
    collinear triangle and the two huge ones."""
    v = qc.scene_q_vertices(np.random.default_rng(11)).reshape(-1, 9)[-64:]
    return write_custom_scene(_dir() / "q_chunk.srt", v)


def vertices_of(path: str) -> np.ndarray:
    return np.array(read_scene(path)[2], f32).reshape(-1, 9)


def bounds(v: np.ndarray):
    """(lo, hi) of the finite vertices; the unit box for a scene without any."""
    p = v.reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        return np.zeros(3, f32), np.ones(3, f32)
    return p.min(axis=0), p.max(axis=0)


def _origins(rng, v, k):
    """Origins inside the scene's bounds: half of them uniform in the bounds, half uniform in the box
    of the 5th to 95th percentile of the vertices (where the triangles are, when a few are huge)."""
    lo, hi = bounds(v)
    p = v.reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    ilo, ihi = (np.percentile(p, 5, axis=0), np.percentile(p, 95, axis=0)) if len(p) else (lo, hi)
    inner = rng.random(k) < 0.5
    o = np.where(inner[:, None], rng.uniform(ilo, ihi, (k, 3)), rng.uniform(lo, hi, (k, 3)))
    return np.clip(o.astype(f32), lo, hi)


def _points_on(rng, v, k):
    """k float32 points on random triangles (a convex combination evaluated in float32) and their ids."""
    n = len(v)
    ids = rng.integers(0, n, k)
    w = rng.dirichlet([1.0, 1.0, 1.0], k).astype(f32)
    tri = v[ids].reshape(k, 3, 3)
    p = (w[:, 0:1] * tri[:, 0] + w[:, 1:2] * tri[:, 1]) + w[:, 2:3] * tri[:, 2]
    return p.astype(f32), ids


def _rays(o, d, tmin=0.0, tmax=np.inf):
    k = len(o)
    r = np.empty((k, 8), f32)
    r[:, 0:3] = o
    r[:, 3] = tmin
    r[:, 4:7] = d
    r[:, 7] = tmax
    return r


def degenerate_rays() -> np.ndarray:
    """Rays that miss whatever the scene: a non-finite origin or direction component, d = 0 (of both
    signs), a NaN range, tmin > tmax."""
    base = np.array([0.1, 0.2, 0.0, 0.0, 0.05, -0.02, 1.0, np.inf], f32)
    out = []
    for col in (0, 1, 2, 4, 5, 6):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[col] = bad
            out.append(r)
    for z in (0.0, -0.0):
        r = base.copy()
        r[4:7] = z
        out.append(r)
    for col in (3, 7):
        r = base.copy()
        r[col] = np.nan
        out.append(r)
    r = base.copy()
    r[3], r[7] = 5.0, 4.0
    out.append(r)
    r = base.copy()
    r[3], r[7] = np.inf, -np.inf
    out.append(r)
    return np.array(out, f32)


def open_sets(path: str, total: int, seed: int) -> dict:
    """The families with tmin = 0, tmax = +inf and origins inside the scene's bounds, about `total`
    rays in all: 'aimed' (at random points of random triangles: most hit), 'random' (directions),
    'axis' (one or two direction components exactly 0 or -0: 20 % of the total), 'surface' (origins
    exactly on triangle surfaces and vertices)."""
    v = vertices_of(path)
    rng = np.random.default_rng(seed)
    k = max(4, total // 5)
    if len(v) == 0:
        o = _origins(rng, v, 4 * k)
        return {"random": _rays(o, rng.normal(size=(4 * k, 3)).astype(f32))}
    sets = {}
    o = _origins(rng, v, 2 * k)
    target, _ = _points_on(rng, v, 2 * k)
    sets["aimed"] = _rays(o, target - o)
    sets["random"] = _rays(_origins(rng, v, k), rng.normal(size=(k, 3)).astype(f32))
    o = _origins(rng, v, k)
    target, _ = _points_on(rng, v, k)
    d = np.where(rng.random((k, 1)) < 0.5, target - o, rng.normal(size=(k, 3)).astype(f32)).astype(f32)
    zero = np.zeros((k, 3), bool)
    zero[np.arange(k), rng.integers(0, 3, k)] = True
    second = rng.random(k) < 0.4
    zero[np.arange(k), rng.integers(0, 3, k)] |= second
    zero[zero.all(axis=1), 0] = False
    d[zero] = np.where(rng.random(int(zero.sum())) < 0.5, f32(0.0), f32(-0.0))
    sets["axis"] = _rays(o, d)
    p, ids = _points_on(rng, v, k)
    corner = rng.random(k) < 0.3
    p[corner] = v[ids[corner]].reshape(-1, 3, 3)[np.arange(int(corner.sum())), rng.integers(0, 3, int(corner.sum()))]
    sets["surface"] = _rays(p, rng.normal(size=(k, 3)).astype(f32))
    return sets


def finite_sets(path: str, total: int, seed: int) -> dict:
    """The families with a range of their own, built on the host's own t of known hits (of
    open_sets' 'aimed' rays): 'lift' (surface origins with tmin = 2^-10), 'exact' (tmin = tmax = t),
    'below' / 'above' (tmax = nextafter(t) either way), 'short' (tmax = t / 2), 'late' (tmin = 2 t)."""
    from simpleraytracer_amd import device

    v = vertices_of(path)
    if len(v) == 0:
        return {}
    sets = open_sets(path, total, seed)
    lift = sets["surface"].copy()
    lift[:, 3] = f32(2.0 ** -10)
    aimed = sets["aimed"]
    ids, t, _ = device.closest_host(path, aimed)
    hit = np.flatnonzero(ids >= 0)
    out = {"lift": lift}
    if hit.size:
        k = max(1, total // 12)
        pick = hit[np.random.default_rng(seed + 1).integers(0, hit.size, 5 * k)].reshape(5, k)
        th = [t[p] for p in pick]
        r = [aimed[p].copy() for p in pick]
        r[0][:, 3], r[0][:, 7] = th[0], th[0]
        r[1][:, 7] = np.nextafter(th[1], -INF)
        r[2][:, 7] = np.nextafter(th[2], INF)
        r[3][:, 7] = th[3] * f32(0.5)
        r[4][:, 3] = th[4] * f32(2.0)
        out.update(exact=r[0], below=r[1], above=r[2], short=r[3], late=r[4])
    return out


@functools.lru_cache(maxsize=None)
def mixed_rays(path: str, total: int, seed: int = 7) -> np.ndarray:
    """Every family of open_sets and finite_sets and the degenerate rays, shuffled: about 1.5 `total` rays."""
    parts = list(open_sets(path, total, seed).values()) + list(finite_sets(path, total, seed).values())
    parts.append(degenerate_rays())
    r = np.concatenate(parts)
    r = np.ascontiguousarray(r[np.random.default_rng(seed + 2).permutation(len(r))])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def host_answers(path: str, total: int, seed: int = 7):
    """(rays, ids, t, bary, occluded): the host path's answers for mixed_rays, computed once."""
    from simpleraytracer_amd import device

    rays = mixed_rays(path, total, seed)
    ids, t, bary = device.closest_host(path, rays)
    occ = device.occluded_host(path, rays)
    for a in (ids, t, bary, occ):
        a.setflags(write=False)
    return rays, ids, t, bary, occ


def assert_mix(ids, large_ids=None):
    """The answers cover what a test relies on: hits, misses and, for scene Q, winners among its two
    huge triangles."""
    n = len(ids)
    assert (ids >= 0).sum() >= 0.10 * n, f"only {(ids >= 0).sum()} of {n} rays hit"
    assert (ids < 0).sum() >= 0.10 * n, f"only {(ids < 0).sum()} of {n} rays miss"
    if large_ids is not None:
        won = ids[ids >= 0]
        assert np.isin(won, large_ids).sum() >= 0.01 * len(won)


def assert_same(got, want):
    """Exact: (ids, t, bary) equal, t and the barycentrics on the uint32 view."""
    qc.assert_same(got[0], got[1], want[0], want[1])
    g, w = np.asarray(got[2], f32).view(np.uint32), np.asarray(want[2], f32).view(np.uint32)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, f"{bad.size} barycentrics differ, first at {bad[0]}"
