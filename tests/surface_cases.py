"""Shared cases of the vertex-attribute tests (test_surface_host.py, test_gpu_surface.py): the numpy
float32 restatement of DESIGN.md section 2 "Vertex attributes", the E_k and det it starts from (the
oracle's, never the library's), random corner tables and textures from fixed seeds, and a
self-check of the specification itself. Not a test module.

Every operation below is a numpy float32 operation -- one rounding each, in the order DESIGN.md
writes it -- so the library's planes must equal the restatement's on the uint32 view.

  E_k, det   as gbuffer_cases.expected obtains them: E_k = the det oracle.closest_hit reports for the
             one-record array (c0_k, cx_k, cy_k, 0, ..., vol = 1); det = (E_A + E_B) + E_C in float32
             must reproduce the bits of the oracle's det for the whole record. Only for pairs that
             hit (ids from the oracle's own scan): the one-record scan answers only for hits.
  fallbacks  without a normals table the normal plane is rtg's (fma arithmetic: gbuffer_cases checks
             it against the oracle with a tolerance), so the restatement gives a normal plane and
             an rgba plane only when there is a normals table; every other plane always.

Self-check of the specification (position_error; run on the CPU, the library takes no part): the
restatement's interpolation of the scene's own vertices (table = the n x 9 vertices, C = 3) is the
hit point; it is compared with eye + t d in float64 (t the oracle's, d from the float32 frame),
relative to |eye| + t |d|. Observed maxima, numpy on the CPU:
    scene Q, 200 x 150, the 'pixels' set   1.07e-4 (its small soup triangles seen nearly edge-on, where
                                           det -- and with it t and the weights -- cancels; 5.8e-7 on
                                           the two frame-covering triangles, 72 % of the hits)
    Cornell, 200 x 150, the 'pixels' set   2.8e-7
The asserted bound is 4 x the observed value: the margin covers a different seed, not platform
variation (both sides are numpy on the CPU).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import gbuffer_cases as gc
import query_cases as qc
from oracle import srt_oracle as oracle

F = np.float32
WRAPS = ("repeat", "clamp")
FILTERS = ("bilinear", "nearest")
TEXTURE_SIZES = ((1, 1), (2, 2), (3, 5), (64, 64))  # (TH, TW): 1 x 1, 2 x 2, 5 x 3 (W x H) and 64 x 64
PLANTED = (0.0, 1.0, -1e-30, np.nan, np.inf, -np.inf)
# The self-check's observed maxima (see the module docstring) and the bound asserted from them.
POSITION_ERROR_OBSERVED = {"q": 1.08e-4, "cornell": 2.9e-7}
POSITION_ERROR_MARGIN = 4.0

same_bits = gc._same_bits


def edge_values(path: str, width: int, height: int, pos: np.ndarray, ids: np.ndarray) -> SimpleNamespace:
    """E_A, E_B, E_C (count x 3) and det (count) of the pairs, float32, and which pairs are inside
    the scene. Every id inside the scene must hit at its position."""
    sc = oracle.OracleScene(path)
    edges = sc.edges(width, height)
    pos = np.asarray(pos, F)
    ids = np.asarray(ids, np.int32)
    valid = (ids >= 0) & (ids < sc.n)
    e = np.zeros((len(ids), 3), F)
    det = np.ones(len(ids), F)
    t = np.full(len(ids), np.inf, F)
    for k in np.flatnonzero(valid):
        i = int(ids[k])
        fx, fy = float(pos[k, 0]), float(pos[k, 1])
        hit, tt, d = oracle.closest_hit(edges[i:i + 1], fx, fy)
        assert hit == 0, f"pair {k}: id {i} does not hit at ({fx}, {fy})"
        e[k] = [gc._edge_value(edges[i, 3 * j:3 * j + 3], fx, fy) for j in range(3)]
        det[k] = F(F(e[k, 0] + e[k, 1]) + e[k, 2])
        assert det[k].view(np.uint32) == F(d).view(np.uint32), f"pair {k}: det not reproduced"
        t[k] = tt
    out = SimpleNamespace(n=sc.n, valid=valid, e=e, det=det, t=t, frame=sc.frame(width, height),
                          albedo=sc.albedo.copy(), background=sc.background.copy(), vertices=sc.vertices.copy(),
                          pos=pos.copy(), ids=ids.copy())
    for a in (out.valid, out.e, out.det, out.t, out.frame, out.albedo, out.background, out.vertices, out.pos, out.ids):
        a.setflags(write=False)
    sc.close()
    return out


@functools.lru_cache(maxsize=None)
def cached_edges(path: str, width: int, height: int, key: str) -> SimpleNamespace:
    """edge_values() of qc.cached_answers' named pair set ('pixels' or 'mixed'), once per session."""
    pos, ids, _ = qc.cached_answers(path, width, height, key)
    return edge_values(path, width, height, pos, ids)


def tables(n: int, seed: int, hit_ids=None) -> SimpleNamespace:
    """Random corner tables of an n-triangle scene: normals (n, 3, 3) in [-1, 1] (not unit), uvs
    (n, 3, 2) in [-1.5, 2.5], generic (n, 3, 4) in [-2, 2]. hit_ids: triangles that are hit; the
    first six of them get the planted uvs -- every corner exactly 0, exactly 1, -1e-30, and one
    corner NaN, +inf, -inf."""
    rng = np.random.default_rng(seed)
    normals = rng.uniform(-1.0, 1.0, (n, 3, 3)).astype(F)
    uvs = rng.uniform(-1.5, 2.5, (n, 3, 2)).astype(F)
    generic = rng.uniform(-2.0, 2.0, (n, 3, 4)).astype(F)
    planted = []
    if hit_ids is not None:
        planted = [int(i) for i in np.unique(np.asarray(hit_ids)[np.asarray(hit_ids) >= 0])[:len(PLANTED)]]
        assert len(planted) == len(PLANTED)
        for i, value in zip(planted, PLANTED):
            if np.isfinite(value):
                uvs[i] = F(value)
            else:
                uvs[i, 1, 0] = F(value)
                uvs[i, 2, 1] = F(value)
    out = SimpleNamespace(normals=normals, uvs=uvs, generic=generic, planted=planted)
    for a in (normals, uvs, generic):
        a.setflags(write=False)
    return out


def texture(th: int, tw: int, seed: int) -> np.ndarray:
    """(th, tw, 4) float32 in [0, 1]; .a random as well (it is ignored)."""
    t = np.random.default_rng(seed).random((th, tw, 4), dtype=F)
    t.setflags(write=False)
    return t


# --- the restatement ---------------------------------------------------------------------------

def weights(ev):
    with np.errstate(all="ignore"):
        return ev.e[:, 0] / ev.det, ev.e[:, 1] / ev.det, ev.e[:, 2] / ev.det


def mix(w, a0, a1, a2):
    """(w0 a0 + w1 a1) + w2 a2 per element; a_k (count,) or (count, C)."""
    w0, w1, w2 = (x if np.ndim(a0) == 1 else x[:, None] for x in w)
    with np.errstate(all="ignore"):
        return (w0 * a0 + w1 * a1) + w2 * a2


def interpolate(ev, table) -> np.ndarray:
    """The interpolation of a corner table (n, 3, C): (count, C) float32, 0 outside the scene."""
    table = np.asarray(table, F)
    rows = table[np.where(ev.valid, ev.ids, 0)]
    out = mix(weights(ev), rows[:, 0], rows[:, 1], rows[:, 2])
    out[~ev.valid] = 0
    assert out.dtype == F
    return out


def dotp(a, b):
    with np.errstate(all="ignore"):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def smooth_normal(ev, normals) -> np.ndarray:
    """The normal plane (count, 4) under a normals table; (0, 0, 0, 1) outside the scene."""
    ns = interpolate(ev, normals)
    base, du, dv = ev.frame[3:6], ev.frame[6:9], ev.frame[9:12]
    fx, fy = ev.pos[:, 0:1], ev.pos[:, 1:2]
    with np.errstate(all="ignore"):
        d = (base[None, :] + fx * du[None, :]) + fy * dv[None, :]
        nn, nd, dd = dotp(ns, ns), dotp(ns, d), dotp(d, d)
        length = np.sqrt(nn)
        c = np.abs(nd) / (length * np.sqrt(dd))
        cos = np.where(c < 1, c, F(1))
        u = ns / length[:, None]
        u = np.where((nd > 0)[:, None], -u, u)
    out = np.concatenate([u, cos[:, None]], axis=1).astype(F)
    out[~ev.valid] = (0, 0, 0, 1)
    return out


def wrap(u, clamp: bool):
    with np.errstate(all="ignore"):
        if clamp:
            return np.where(u > 0, np.where(u < 1, u, F(1)), F(0)).astype(F)
        r = u - np.floor(u)
        return np.where((r >= 0) & (r <= 1), r, F(0)).astype(F)


def taps(r, size: int, clamp: bool):
    """(i0, i1, a, path) of the bilinear filter on one axis; path 0: no wrap, 1: i0 wrapped (or
    clamped), 2: i1 wrapped (or clamped)."""
    x = r * F(size) - F(0.5)
    x0 = np.floor(x)
    a = x - x0
    i0 = x0.astype(np.int32)
    i1 = i0 + 1
    path = np.where(i0 < 0, 1, np.where(i1 >= size, 2, 0))
    if clamp:
        i0, i1 = np.maximum(i0, 0), np.minimum(i1, size - 1)
    else:
        i0, i1 = np.where(i0 < 0, i0 + size, i0), np.where(i1 >= size, i1 - size, i1)
    assert a.dtype == F and i0.min() >= 0 and i1.max() < size and i1.min() >= 0 and i0.max() < size
    return i0, i1, a, path


def nearest(r, size: int):
    return np.minimum(np.floor(r * F(size)).astype(np.int32), size - 1)


def lookup(tex, uv, wrap_mode: str, filter_mode: str):
    """tex.rgb at uv (count, 2): (count, 3) float32, and the u-axis and v-axis tap paths (None for
    the nearest filter)."""
    th, tw = tex.shape[:2]
    clamp = wrap_mode == "clamp"
    ru, rv = wrap(uv[:, 0], clamp), wrap(uv[:, 1], clamp)
    t = np.asarray(tex, F)[..., :3]
    if filter_mode == "nearest":
        return t[nearest(rv, th), nearest(ru, tw)], None, None
    i0, i1, a, pu = taps(ru, tw, clamp)
    j0, j1, b, pv = taps(rv, th, clamp)
    a, b = a[:, None], b[:, None]
    top = t[j0, i0] + a * (t[j0, i1] - t[j0, i0])
    bot = t[j1, i0] + a * (t[j1, i1] - t[j1, i0])
    out = top + b * (bot - top)
    assert out.dtype == F
    return out, pu, pv


def expected(ev, normals=None, uvs=None, tex=None, wrap_mode="repeat", filter_mode="bilinear", modulate=False):
    """The planes of a surface call on the pairs of `ev`: uv and albedo always, normal and rgba when
    there is a normals table (see the module docstring), and the tap paths of a bilinear lookup."""
    count = len(ev.ids)
    hit = ev.valid
    out = SimpleNamespace(normal=None, rgba=None, paths=None)
    out.uv = interpolate(ev, uvs) if uvs is not None else np.zeros((count, 2), F)
    rgb = ev.albedo[np.where(hit, ev.ids, 0)].astype(F)
    if tex is not None:
        texel, pu, pv = lookup(tex, out.uv, wrap_mode, filter_mode)
        rgb = texel * rgb if modulate else texel
        out.paths = None if pu is None else (pu[hit], pv[hit])
    albedo = np.concatenate([rgb, ev.ids.astype(F)[:, None]], axis=1).astype(F)
    albedo[~hit] = (*ev.background, -1.0)
    out.albedo = albedo
    if normals is not None:
        out.normal = smooth_normal(ev, normals)
        out.rgba = np.concatenate([albedo[:, :3] * out.normal[:, 3:], albedo[:, 3:]], axis=1).astype(F)
    return out


def check_surface(exp, normal, albedo, rgba, uv):
    """The planes of a surface call against expected(): on the bits."""
    same_bits("uv", uv, exp.uv)
    same_bits("albedo", albedo, exp.albedo)
    if exp.normal is not None:
        same_bits("normal", normal, exp.normal)
        same_bits("rgba", rgba, exp.rgba)


def miss_planes(count: int, background):
    """(normal, albedo, rgba, uv) of `count` ids outside the scene."""
    px = np.tile(F([*background, -1.0]), (count, 1))
    return np.tile(F([0, 0, 0, 1]), (count, 1)), px, px.copy(), np.zeros((count, 2), F)


# --- the self-check of the specification --------------------------------------------------------

def position_error(path: str, width: int, height: int, key: str = "pixels") -> float:
    """max over the hit pairs of |P32 - P64| / (|eye| + t |d|): P32 the restatement's interpolation
    of the scene's own vertices, P64 = eye + t d in float64."""
    ev = cached_edges(path, width, height, key)
    hit = ev.valid
    assert hit.sum() >= 1000
    p32 = interpolate(ev, ev.vertices.reshape(-1, 3, 3))[hit].astype(np.float64)
    fr = ev.frame.astype(np.float64)
    eye, base, du, dv = fr[0:3], fr[3:6], fr[6:9], fr[9:12]
    pos = ev.pos[hit].astype(np.float64)
    d = base[None, :] + pos[:, 0:1] * du[None, :] + pos[:, 1:2] * dv[None, :]
    t = ev.t[hit].astype(np.float64)[:, None]
    p64 = eye[None, :] + t * d
    scale = np.linalg.norm(eye) + t[:, 0] * np.linalg.norm(d, axis=1)
    return float((np.linalg.norm(p32 - p64, axis=1) / scale).max())


def check_position_error(path: str, width: int, height: int, name: str) -> float:
    got = position_error(path, width, height)
    bound = POSITION_ERROR_MARGIN * POSITION_ERROR_OBSERVED[name]
    print(f"surface_cases: interpolated position error on {name}: {got:.3e} (bound {bound:.3e})")
    assert got <= bound, f"{name}: interpolated position off by {got:.3e} relative, bound {bound:.3e}"
    return got
