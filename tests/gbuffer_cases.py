"""Shared cases of the G-buffer tests (test_gbuffer_host.py, test_gpu_gbuffer.py): the expected
surface attributes of (position, id) pairs, from the oracle and numpy -- never from the library --
and the checks of the four planes against them. Not a test module.

Expected values (DESIGN.md section 2 "Surface attributes"):
  depth    oracle.closest_hit over the one record of the id: its t, compared on the uint32 view.
  bary     E_k = the det oracle.closest_hit reports for the one-record array (c0_k, cx_k, cy_k, 0...,
           vol = 1): the other two edge values are fma(fy, 0, fma(fx, 0, 0)) = 0 for finite
           positions (a miss: E_k = 0). det = (E_A + E_B) + E_C in float32 must reproduce the
           oracle's det; w = E_k / det in float32, bit-exact.
  albedo   the scene file's albedo of the id, bit-exact; .a == float(id).
  normal   N32 = cross(v1 - v0, v2 - v0) in float32 (no fma: the canonical N's bits), normalised in
           float64; 2^-22 absolute per component (dot3(N, N): three roundings of a sum of squares,
           so |N| is within 2.5 * 2^-24 relative after the root; the division adds 2^-24). Sign:
           -sign(N32 . d) in float64 wherever |cos| > 1e-6 (the float error of nd is below
           3.2e-7 |N| |d|); either sign below that.
  miss     (+inf, (0, 0), (0, 0, 0, 1), (background, -1)) for every id outside [0, n).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import query_cases as qc
from oracle import srt_oracle as oracle

MISS_IDS = (-1, -7, None, 2**31 - 1, -2**31)  # None: n, the first id past the scene
NORMAL_TOL = 2.0 ** -22


def miss_ids(n: int) -> np.ndarray:
    return np.array([n if i is None else i for i in MISS_IDS], np.int64).astype(np.int32)


def _edge_value(c3, fx, fy) -> np.float32:
    rec = np.zeros((1, 12), np.float32)
    rec[0, 0:3] = c3
    rec[0, 9] = 1.0
    i, _, det = oracle.closest_hit(rec, fx, fy)
    return np.float32(det) if i >= 0 else np.float32(0.0)


def expected(path: str, width: int, height: int, pos: np.ndarray, ids: np.ndarray) -> SimpleNamespace:
    """The expected planes of the pairs (pos[k], ids[k]). Every id inside the scene must be a hit at
    its position (ids from a trace or a query): the oracle's one-record scan answers only for hits."""
    sc = oracle.OracleScene(path)
    n = sc.n
    edges = sc.edges(width, height)
    frame = sc.frame(width, height).astype(np.float64)
    base, du, dv = frame[3:6], frame[6:9], frame[9:12]
    pos = np.asarray(pos, np.float32)
    ids = np.asarray(ids, np.int32)
    count = len(ids)
    valid = (ids >= 0) & (ids < n)
    depth = np.full(count, np.inf, np.float32)
    bary = np.zeros((count, 2), np.float32)
    albedo = np.empty((count, 4), np.float32)
    albedo[:, :3] = sc.background
    albedo[:, 3] = -1.0
    unit = np.zeros((count, 3), np.float64)  # the unsigned unit normal, float64
    cos64 = np.ones(count, np.float64)       # N32 . d / (|N32| |d|), signed, float64
    for k in np.flatnonzero(valid):
        i = int(ids[k])
        fx, fy = float(pos[k, 0]), float(pos[k, 1])
        hit, t, det = oracle.closest_hit(edges[i:i + 1], fx, fy)
        assert hit == 0, f"pair {k}: id {i} does not hit at ({fx}, {fy})"
        e = [_edge_value(edges[i, 3 * j:3 * j + 3], fx, fy) for j in range(3)]
        d32 = np.float32(np.float32(e[0] + e[1]) + e[2])
        assert d32.view(np.uint32) == np.float32(det).view(np.uint32), f"pair {k}: det not reproduced"
        depth[k] = t
        bary[k] = (e[1] / d32, e[2] / d32)
        albedo[k, :3] = sc.albedo[i]
        albedo[k, 3] = np.float32(i)
        v = sc.vertices[i].reshape(3, 3)
        n32 = np.cross(v[1] - v[0], v[2] - v[0])
        assert n32.dtype == np.float32
        n64 = n32.astype(np.float64)
        unit[k] = n64 / np.linalg.norm(n64)
        d = base + np.float64(pos[k, 0]) * du + np.float64(pos[k, 1]) * dv
        cos64[k] = unit[k] @ d / np.linalg.norm(d)
    assert bary.dtype == np.float32
    out = SimpleNamespace(n=n, count=count, valid=valid, depth=depth, bary=bary, albedo=albedo, unit=unit, cos64=cos64,
                          background=sc.background.copy())
    for a in (valid, depth, bary, albedo, unit, cos64):
        a.setflags(write=False)
    sc.close()
    return out


def _same_bits(name, got, want):
    g = np.ascontiguousarray(got, np.float32).view(np.uint32).reshape(-1)
    w = np.ascontiguousarray(want, np.float32).view(np.uint32).reshape(-1)
    assert g.shape == w.shape, f"{name}: shape {np.shape(got)} != {np.shape(want)}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{name}: {bad.size} values differ, first at {bad[0]}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"


def check_planes(exp, depth=None, bary=None, normal=None, albedo=None):
    """The planes given against the expected values of `exp` (expected())."""
    hit = exp.valid
    if depth is not None:
        _same_bits("depth", np.reshape(depth, -1), exp.depth)
    if bary is not None:
        _same_bits("bary", np.reshape(bary, (-1, 2)), exp.bary)
    if albedo is not None:
        _same_bits("albedo", np.reshape(albedo, (-1, 4)), exp.albedo)
    if normal is not None:
        nm = np.reshape(normal, (-1, 4)).astype(np.float64)
        assert nm.shape[0] == exp.count
        miss = nm[~hit]
        assert np.all(miss == np.array([0.0, 0.0, 0.0, 1.0])), "a miss's normal is (0, 0, 0, 1)"
        got = nm[hit]
        unit, c = exp.unit[hit], exp.cos64[hit]
        # turned towards the eye: s = -sign(N . d); either sign where |cos| <= 1e-6
        s = np.where(c > 0, -1.0, 1.0)[:, None]
        err = np.abs(got[:, :3] - s * unit).max(axis=1)
        err_other = np.abs(got[:, :3] + s * unit).max(axis=1)
        free = np.abs(c) <= 1e-6
        err = np.where(free, np.minimum(err, err_other), err)
        bad = np.flatnonzero(err > NORMAL_TOL)
        assert bad.size == 0, f"normal: {bad.size} off by more than 2^-22, worst {err.max():.3e}"
        # .w is the shading cosine, |cos| <= 1 (the exact value is checked through the RGBA identity)
        assert np.all(np.abs(got[:, 3] - np.minimum(np.abs(c), 1.0)) <= 1e-5)


def check_misses(ids, n, background, depth, bary, normal, albedo):
    """Every id outside [0, n): the miss values, on the bits."""
    ids = np.asarray(ids).reshape(-1)
    miss = (ids < 0) | (ids >= n)
    k = int(miss.sum())
    _same_bits("miss depth", np.reshape(depth, -1)[miss], np.full(k, np.inf, np.float32))
    _same_bits("miss bary", np.reshape(bary, (-1, 2))[miss], np.zeros((k, 2), np.float32))
    _same_bits("miss normal", np.reshape(normal, (-1, 4))[miss], np.tile(np.float32([0, 0, 0, 1]), (k, 1)))
    want = np.tile(np.float32([*background, -1.0]), (k, 1))
    _same_bits("miss albedo", np.reshape(albedo, (-1, 4))[miss], want)


def composed_rgba(normal, albedo) -> np.ndarray:
    """albedo.rgb * normal.w, albedo.a: the RGBA pixel the traces store (float32 products)."""
    nm = np.asarray(normal, np.float32)
    al = np.asarray(albedo, np.float32)
    out = np.empty(al.shape, np.float32)
    out[..., :3] = al[..., :3] * nm[..., 3:]
    out[..., 3] = al[..., 3]
    return out


def check_identity(normal, albedo, rgba):
    """Bit-equal to a traced RGBA frame of the same offsets."""
    _same_bits("albedo.rgb * normal.w, albedo.a", composed_rgba(normal, albedo), rgba)


def check_shade(path, width, height, offsets, ids, normal, albedo):
    """Within 1e-5 (the project's shading tolerance) of oracle.shade of the same whole frame."""
    sc = oracle.OracleScene(path)
    want = sc.shade(width, height, np.reshape(ids, (height, width)), offsets)
    sc.close()
    got = composed_rgba(np.reshape(normal, (height, width, 4)), np.reshape(albedo, (height, width, 4)))
    assert np.array_equal(got[..., 3], want[..., 3])
    assert float(np.abs(got[..., :3] - want[..., :3]).max()) <= 1e-5


@functools.lru_cache(maxsize=None)
def cached_expected(path: str, width: int, height: int, key: str):
    """expected() of a named pair set of a scene, once per session: qc.cached_answers' positions
    ('pixels' or 'mixed') with the oracle's own ids."""
    pos, ids, t = qc.cached_answers(path, width, height, key)
    exp = expected(path, width, height, pos, ids)
    _same_bits("the one-record depth equals the full scan's", exp.depth, t)
    return pos, ids, exp
