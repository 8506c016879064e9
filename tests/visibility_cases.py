"""Shared cases of the sampled-visibility tests (test_visibility_host.py, test_gpu_visibility.py):
the scenes, the frames, the generators with fixed seeds, the numpy float32 restatement of DESIGN.md
section 2 "Visibility" and the host's answers, computed once and shared read-only. Not a test module.

The restatement takes the frame and the edge records from the oracle, the depth's three fused edge
values from the oracle's own scan (one record at a time), and evaluates everything else in numpy
float32 arrays, one rounding per operation."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import query_cases as qc
import rays_cases as rc
from oracle import srt_oracle as oracle

f32 = np.float32
FRAMES = ((48, 32), (70, 33))  # 70 x 33: no multiple of the wave width, of the block or of its tile
TMIN = 2.0 ** -10
SENTINEL = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def scene_path(name: str) -> str:
    import simpleraytracer_amd as srt

    if name == "q":
        return rc.q_path()
    if name == "cornell":
        return srt.write_scene(str(rc._dir() / "visibility_cornell.srt"), "cornell")
    assert name == "soup"
    return rc.soup_path(2000)


def offsets_of(w: int, h: int, jitter: bool) -> np.ndarray:
    return qc.random_offsets(w, h, 9) if jitter else np.full((h, w, 2), 0.5, f32)


@functools.lru_cache(maxsize=None)
def frame_elements(name: str, w: int, h: int, jitter: bool):
    """(offsets (h, w, 2), positions (h w, 2), ids (h w,)) of a scene's frame: the host query's hit ids."""
    from simpleraytracer_amd import device

    off = offsets_of(w, h, jitter)
    pos = device.pixel_positions(w, h, off)
    ids, _ = device.query_host(scene_path(name), w, h, pos)
    for a in (off, pos, ids):
        a.setflags(write=False)
    return off, pos, ids


def hemisphere(samples: int, tmax: float, rotations=None, seed: int = 3, tmin: float = TMIN):
    from simpleraytracer_amd import device
    from simpleraytracer_amd import samples as sm

    rot = sm.rotations(seed + 50) if rotations is True else rotations
    return device.Hemisphere(sm.cosine_hemisphere(samples, seed), tmin, tmax, rot)


def area_light(samples: int, seed: int = 3):
    from simpleraytracer_amd import device
    from simpleraytracer_amd import samples as sm

    return device.AreaLight((-0.3, 1.5, 2.7), (0.6, 0.0, 0.0), (0.0, 0.0, 0.6), sm.area_samples(samples, seed))


def mirror():
    from simpleraytracer_amd import device

    return device.Mirror()


# name -> (scene, generator factory): the three mixes of the issue's table, S = 8 unless asked otherwise
MIXES = {
    "cornell_hemisphere": ("cornell", lambda s=8, rot=None: hemisphere(s, 1.0, rot)),
    "soup_hemisphere": ("soup", lambda s=8, rot=None: hemisphere(s, 0.3, rot)),
    "soup_area": ("soup", lambda s=8, rot=None: area_light(s)),
}


def to_device(gen, dev: str = "cuda:0"):
    """The generator over device tensors of the same tables."""
    import torch

    from simpleraytracer_amd import device

    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, f32)).to(dev)

    if isinstance(gen, device.Hemisphere):
        return device.Hemisphere(up(gen.samples), gen.tmin, gen.tmax, up(gen.rotations))
    if isinstance(gen, device.AreaLight):
        return device.AreaLight(tuple(gen.corner), tuple(gen.eu), tuple(gen.ev), up(gen.samples), gen.tmin, gen.tmax)
    return device.Mirror(gen.tmin, gen.tmax)


def frame_turns(w: int, h: int) -> np.ndarray:
    """The rotation index of every pixel of a frame call, row-major: ((y & 3) << 2) | (x & 3)."""
    y, x = np.mgrid[0:h, 0:w]
    return (((y & 3) << 2) | (x & 3)).reshape(-1)


def _per_turn(gen, turns, call):
    """A host call for elements whose rotation index is `turns` rather than i & 15: the elements of
    each index in a call of their own, with a table that holds that rotation 16 times."""
    from simpleraytracer_amd import device

    if getattr(gen, "rotations", None) is None:
        return call(gen, slice(None)), None
    parts = {}
    for k in np.unique(turns):
        one = device.Hemisphere(gen.samples, gen.tmin, gen.tmax, np.tile(gen.rotations[k], (16, 1)))
        parts[int(k)] = call(one, np.flatnonzero(turns == k))
    return None, parts


def host_visibility(path, w, h, pos, ids, gen, turns=None):
    """(visible, fraction) of the host path; turns: the elements' rotation indices (a frame call's),
    None: a points call's i & 15."""
    from simpleraytracer_amd import device

    if turns is None or getattr(gen, "rotations", None) is None:
        return device.visibility_host(path, w, h, pos, ids, gen)
    visible, fraction = np.empty(len(ids), np.uint8), np.empty(len(ids), f32)
    _, parts = _per_turn(gen, turns, lambda g, sel: (sel, device.visibility_host(path, w, h, pos[sel], ids[sel], g)))
    for sel, (v, f) in parts.values():
        visible[sel], fraction[sel] = v, f
    return visible, fraction


def host_rays(path, w, h, pos, ids, gen, turns=None):
    """(S, count, 8) rays of the host path; turns as host_visibility's."""
    from simpleraytracer_amd import device

    if turns is None or getattr(gen, "rotations", None) is None:
        return device.rays_host(path, w, h, pos, ids, gen)
    rays = np.empty((gen.count, len(ids), 8), f32)
    _, parts = _per_turn(gen, turns, lambda g, sel: (sel, device.rays_host(path, w, h, pos[sel], ids[sel], g)))
    for sel, r in parts.values():
        rays[:, sel] = r
    return rays


@functools.lru_cache(maxsize=None)
def mix_answer(mix: str, w: int, h: int, jitter: bool, samples: int = 8, rot: bool = False):
    """(gen, visible, fraction) of the host for a mix's whole frame (frame-call rotation indices),
    computed once per session."""
    name, make = MIXES[mix]
    _, pos, ids = frame_elements(name, w, h, jitter)
    gen = make(samples, True if rot else None)
    visible, fraction = host_visibility(scene_path(name), w, h, pos, ids, gen, frame_turns(w, h))
    visible.setflags(write=False)
    fraction.setflags(write=False)
    return gen, visible, fraction


def assert_mix(visible, ids, n, samples):
    """The host answer covers what a test relies on: at least three distinct values of `visible` each
    on >= 5 % of the surface elements, visible = S occurs, visible <= S / 2 occurs."""
    surface = (ids >= 0) & (ids < n)
    v = np.asarray(visible)[surface]
    assert v.size > 0
    hist = np.bincount(v, minlength=samples + 1)
    assert (hist >= 0.05 * v.size).sum() >= 3, f"histogram {hist.tolist()}"
    assert hist[samples] > 0, f"visible = S does not occur: {hist.tolist()}"
    assert hist[:samples // 2 + 1].sum() > 0, f"visible <= S / 2 does not occur: {hist.tolist()}"


def same_bits(name, got, want):
    g = np.ascontiguousarray(got, f32).view(np.uint32).reshape(-1)
    w = np.ascontiguousarray(want, f32).view(np.uint32).reshape(-1)
    assert g.shape == w.shape, f"{name}: shape {np.shape(got)} != {np.shape(want)}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{name}: {bad.size} values differ, first at {bad[0]}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"


def fraction_of(visible, samples):
    return np.asarray(visible).astype(f32) / f32(samples)


# ---------------------------------------------------------------------------------------------
# The numpy restatement
# ---------------------------------------------------------------------------------------------

def _edge_value(c3, fx, fy) -> np.float32:
    """fma(fy, cy, fma(fx, cx, c0)) from the oracle's scan of the one record (c3, 0, 0; vol 0): it
    reports det = E for E > 0; the negated record reports -E (fma is odd in c); neither: E = 0."""
    rec = np.zeros((1, 12), f32)
    for sign in (f32(1), f32(-1)):
        rec[0, 0:3] = sign * c3
        i, _, det = oracle.closest_hit(rec, fx, fy)
        if i >= 0:
            return sign * f32(det)
    return f32(0.0)


def dotp(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def restate_rays(path: str, w: int, h: int, pos, ids, gen, turns=None) -> np.ndarray:
    """DESIGN.md section 2 "Visibility", steps 1 to 5, in numpy float32: (S, count, 8) rays."""
    from simpleraytracer_amd import _native

    s = oracle.OracleScene(path)
    n, edges, fr, v = s.n, s.edges(w, h), s.frame(w, h), s.vertices.astype(f32)
    s.close()
    eye, base, du, dv = fr[0:3], fr[3:6], fr[6:9], fr[9:12]
    pos, ids = np.asarray(pos, f32), np.asarray(ids, np.int32)
    count, S = len(ids), gen.count
    inside = (ids >= 0) & (ids < n)
    safe = np.where(inside, ids, 0)
    t = np.full(count, np.nan, f32)
    with np.errstate(all="ignore"):
        for k in np.flatnonzero(inside):
            rec = edges[ids[k]]
            fx, fy = float(pos[k, 0]), float(pos[k, 1])
            if np.isnan(rec[9]):
                continue
            e = [_edge_value(rec[3 * j:3 * j + 3], fx, fy) for j in range(3)]
            t[k] = rec[9] / f32(f32(e[0] + e[1]) + e[2])
        fx, fy = pos[:, 0:1], pos[:, 1:2]
        d = (base[None] + fx * du[None]) + fy * dv[None]
        P = eye[None] + t[:, None] * d
        tri = v[safe].reshape(count, 3, 3) if n else np.zeros((count, 3, 3), f32)
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
        nn, nd = dotp(N, N), dotp(N, d)
        valid = inside & np.isfinite(t) & np.isfinite(nn) & (nn > 0)
        nrm = N / np.sqrt(nn)[:, None]
        nrm = np.where((nd > 0)[:, None], -nrm, nrm)
        assert d.dtype == P.dtype == nrm.dtype == f32
        rays = np.zeros((S, count, 8), f32)
        if gen.kind == _native.RTA_HEMISPHERE:
            nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
            sg = np.where(nz < 0, f32(-1), f32(1))
            a = f32(-1) / (sg + nz)
            b = (nx * ny) * a
            T = np.stack([f32(1) + ((sg * nx) * nx) * a, sg * b, (-sg) * nx], -1)
            B = np.stack([b, sg + (ny * ny) * a, -ny], -1)
            table = np.asarray(gen.samples, f32)
            if gen.rotations is not None:
                turn = (np.arange(count) & 15) if turns is None else turns
                c, sn = np.asarray(gen.rotations, f32)[turn, 0], np.asarray(gen.rotations, f32)[turn, 1]
            for i in range(S):
                lx, ly, lz = table[i]
                if gen.rotations is not None:
                    rx, ry = lx * c - ly * sn, lx * sn + ly * c
                else:
                    rx, ry = np.full(count, lx, f32), np.full(count, ly, f32)
                rays[i, :, 4:7] = (rx[:, None] * T + ry[:, None] * B) + lz * nrm
        elif gen.kind == _native.RTA_AREA:
            corner, eu, ev = (np.array(list(x), f32) for x in (gen.corner, gen.eu, gen.ev))
            table = np.asarray(gen.samples, f32)
            for i in range(S):
                L = (corner + table[i, 0] * eu) + table[i, 1] * ev
                rays[i, :, 4:7] = L[None] - P
        else:
            dn = dotp(d, nrm)
            rays[0, :, 4:7] = d - (f32(2) * dn)[:, None] * nrm
        rays[:, :, 0:3] = P[None]
        rays[:, :, 3] = f32(gen.tmin)
        rays[:, :, 7] = f32(gen.tmax)
        rays[:, ~valid] = 0
    assert rays.dtype == f32
    return rays


def points_case(name: str, w: int, h: int, seed: int = 17) -> SimpleNamespace:
    """Points elements of a scene: 600 random positions with the host query's ids, then the ids the
    definition's steps 1 and 3 are about -- -1, n, a large sentinel, scene Q's point and collinear
    triangles where the scene has them -- and ids that do not hit at their position."""
    from simpleraytracer_amd import device

    path = scene_path(name)
    n = device.scene_triangles(path)
    rng = np.random.default_rng(seed)
    pos = rng.random((600, 2), dtype=f32)
    ids, _ = device.query_host(path, w, h, pos)
    extra_ids = [-1, n, SENTINEL, -2 ** 31]
    if name == "q":
        extra_ids += [qc.N_SOUP + 20, qc.N_SOUP + 21]  # the point and the collinear triangle
    extra_ids += [int(i) for i in rng.integers(0, n, 40)]  # (most do not hit where they are asked)
    extra_pos = rng.random((len(extra_ids), 2), dtype=f32)
    pos = np.concatenate([pos, extra_pos])
    ids = np.concatenate([ids, np.array(extra_ids, np.int64).astype(np.int32)])
    return SimpleNamespace(path=path, n=n, pos=pos, ids=ids, special=len(extra_ids))
