"""Shared cases of the sampled-radiance tests (test_radiance_host.py, test_gpu_radiance.py): the
scenes, lights and generators, and the oracle -- the host composition DESIGN.md section 2 "Radiance"
defines the answer as: device.rays_host -> device.closest_host -> device.light_hits_host, then steps
4 to 6 in numpy float32 with a Python loop over the samples. Built on lighting_cases,
visibility_cases, hits_cases and count_cases without touching them. Not a test module.

The main case is the 160 x 96 frame of lighting case T4 (an open scene under four spot lights) with
a hemisphere of S = 3, no rotation. Counts out of 15 360 elements (CPU, the oracle alone): 9 204
without a surface, 759 with 0 < hits < S, 39 with hits == S, 796 with a sample lit by a light, 640
with a sample shadowed, 798 whose mean differs from c_0; summing in descending s changes 300 of the
46 080 sums' bits. (With S = 8 only 8 elements have every ray hit: the scene is open.)
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import count_cases as cc
import lighting_cases as lc
import shadow_cases as sc
import visibility_cases as vc

f32 = np.float32
AMBIENT = lc.AMBIENT
INF = float("inf")
MAIN = ("T4", 3, False)  # lighting case, S, rotations
MAIN_COUNTS = dict(no_surface=9204, partial=759, full=39, lit=796, shadowed=640, mean_differs=798, order_bits=300)


def same_bits(name, got, want):
    vc.same_bits(name, got, want)


def albedo_of(path: str) -> np.ndarray:
    from simpleraytracer_amd import device

    return np.ascontiguousarray(device.read_scene(path)["albedo"], f32)


def samples_of(path, w, h, lights, ambient, pos, ids, gen, turns=None) -> SimpleNamespace:
    """Steps 1 to 3 through the three families' host calls: rays (S, count, 8), ids and t (S, count),
    c (S, count, 4) unblended, classes (L, S, count), on (count,): the element is on a surface (its
    rays are not the eight zeros; every generator here has tmin > 0)."""
    from simpleraytracer_amd import device

    rays = vc.host_rays(path, w, h, pos, ids, gen, turns)
    S, count = rays.shape[0], rays.shape[1]
    flat = np.ascontiguousarray(rays.reshape(-1, 8))
    hid, t, _ = device.closest_host(path, flat)
    c, classes = device.light_hits_host(path, lc.host_lights(lights), ambient, flat, hid, t, classes=True)
    return SimpleNamespace(rays=rays, ids=hid.reshape(S, count), t=t.reshape(S, count), c=c.reshape(S, count, 4),
                           classes=classes.reshape(len(lights), S, count), on=(rays[0] != 0).any(axis=1))


def resolve(sm, path, ids, modulate=False, base=None, weight=(1.0, 1.0, 1.0), descending=False) -> np.ndarray:
    """Steps 4 to 6 in numpy float32, one rounding per operation, the samples in a Python loop."""
    S, count = sm.c.shape[0], sm.c.shape[1]
    total = np.zeros((count, 3), f32)
    with np.errstate(all="ignore"):
        for s in (reversed(range(S)) if descending else range(S)):
            total = total + sm.c[s, :, :3]
            assert total.dtype == f32
        hits = (sm.c[..., 3] >= 0).sum(axis=0)
        m = total / f32(S)
        assert m.dtype == f32
        if modulate:
            alb = albedo_of(path)[np.where(sm.on, ids, 0)]
            m = alb * m
            assert m.dtype == f32
        out = np.zeros((count, 4), f32)
        out[sm.on, :3] = m[sm.on]
        out[sm.on, 3] = (hits.astype(f32) / f32(S))[sm.on]
        if base is not None:
            b = np.asarray(base, f32).reshape(count, 4)
            mixed = b[:, :3] + (np.asarray(weight, f32)[None, :] * out[:, :3]).astype(f32)
            assert mixed.dtype == f32
            out = np.array(b)
            out[sm.on, :3] = mixed[sm.on]
    return out


def oracle(path, w, h, lights, ambient, pos, ids, gen, turns=None, **store) -> np.ndarray:
    return resolve(samples_of(path, w, h, lights, ambient, pos, ids, gen, turns), path, ids, **store)


def host(path, w, h, lights, ambient, pos, ids, gen, turns=None, modulate=False, base=None, weight=(1.0, 1.0, 1.0)):
    """device.radiance_host; turns: the elements' rotation indices (a frame call's) -- the host call
    is a points call, so the elements of each index go in a call of their own whose table holds that
    rotation sixteen times (visibility_cases' way)."""
    from simpleraytracer_amd import device

    hl = lc.host_lights(lights)
    if turns is None or getattr(gen, "rotations", None) is None:
        return device.radiance_host(path, w, h, hl, ambient, pos, ids, gen, modulate=modulate, base=base, weight=weight)
    out = np.empty((len(ids), 4), f32)
    for k in np.unique(turns):
        sel = np.flatnonzero(turns == k)
        one = device.Hemisphere(gen.samples, gen.tmin, gen.tmax, np.tile(gen.rotations[k], (16, 1)))
        out[sel] = device.radiance_host(path, w, h, hl, ambient, pos[sel], ids[sel], one, modulate=modulate,
                                        base=None if base is None else np.asarray(base, f32).reshape(-1, 4)[sel],
                                        weight=weight)
    return out


def base_of(count: int, seed: int = 11) -> np.ndarray:
    """A base picture: random colours, alphas that are no valid answer's."""
    rng = np.random.default_rng(seed)
    b = rng.random((count, 4), dtype=f32)
    b[:, 3] = f32(100.0) + np.arange(count, dtype=f32)
    return b


# --- the cases ------------------------------------------------------------------------------------

def frame_case(name: str, samples: int, rot: bool, tmax: float = INF, seed: int = 3) -> SimpleNamespace:
    """A lighting case's 160 x 96 frame as radiance elements under a hemisphere."""
    from simpleraytracer_amd import device

    c = lc.case(name)
    pos = device.pixel_positions(lc.W, lc.H, c.offsets)
    ids = np.ascontiguousarray(c.ids.reshape(-1))
    return SimpleNamespace(path=c.view, w=lc.W, h=lc.H, lights=c.lights, offsets=c.offsets, pos=pos, ids=ids, n=c.n,
                           gen=vc.hemisphere(samples, tmax, True if rot else None, seed=seed),
                           turns=vc.frame_turns(lc.W, lc.H))


def main_case() -> SimpleNamespace:
    return frame_case(*MAIN)


CORNELL_LIGHTS = (lc.spot((0.4, 1.2, 0.6, 0.0, 0.6, 2.7, 0.0, 1.0, 0.0, 70.0), 64, 48, (1.0, 0.9, 0.8), 0.0, 2.0 ** -7),
                  lc.point((0.0, 1.0, 2.7), 32, (0.3, 0.5, 0.9), 2.0, 2.0 ** -7))


def small_case(name: str, w: int, h: int, samples: int, rot: bool, tmax: float, jitter: bool = True,
               mirror: bool = False) -> SimpleNamespace:
    """visibility_cases' scene `name` ("cornell", "soup", "q") at w x h under CORNELL_LIGHTS."""
    from simpleraytracer_amd import device

    path = vc.scene_path(name)
    off, pos, ids = vc.frame_elements(name, w, h, jitter)
    gen = vc.mirror() if mirror else vc.hemisphere(samples, tmax, True if rot else None)
    return SimpleNamespace(path=path, w=w, h=h, lights=list(CORNELL_LIGHTS), offsets=off, pos=pos, ids=ids,
                           n=device.scene_triangles(path), gen=gen, turns=vc.frame_turns(w, h))


@functools.lru_cache(maxsize=None)
def host_frame(kind: str, *args) -> np.ndarray:
    """radiance_host of a case's whole frame with the frame call's rotation indices, once per session:
    kind "frame" (frame_case's arguments) or "small" (small_case's)."""
    c = frame_case(*args) if kind == "frame" else small_case(*args)
    out = host(c.path, c.w, c.h, c.lights, AMBIENT, c.pos, c.ids, c.gen, c.turns)
    out.setflags(write=False)
    return out


COUNT_LIGHTS = (lc.spot(cc.L1, 64, 64, cc.LIGHT_COLORS[0], 0.0, 2.0 ** -7),
                lc.point(cc.POINT_ORIGIN, 32, cc.LIGHT_COLORS[2], 9.0, 2.0 ** -7))


@functools.lru_cache(maxsize=None)
def count_case(n: int) -> SimpleNamespace:
    """32 point elements of count_cases' scene of n triangles on its 256 x 144 frame: 28 pixels that
    the oracle's frame gives a surface -- first those (at most 14) of which the oracle's composition
    says that a ray hits something, then others --, then ids -1, n, 0 and n - 1 at random positions.
    `hitting` is how many of the 28 have a ray that hits."""
    from simpleraytracer_amd import device

    c = cc.case(cc.name_of(n))
    rng = np.random.default_rng(n)
    gen = vc.hemisphere(8, INF, None)  # (no rotation: an element's rays do not depend on its index in a call)
    frame_ids = cc.frame_ids(c.name).reshape(-1)
    at = np.flatnonzero(frame_ids >= 0)
    at = at[rng.permutation(at.size)[:600]]
    where = device.pixel_positions(cc.W, cc.H, cc.offsets(cc.W, cc.H))[at]
    sm = samples_of(c.path, cc.W, cc.H, [], AMBIENT, where, frame_ids[at], gen)
    hit = sm.on & (sm.ids >= 0).any(axis=0)
    first = np.flatnonzero(hit)[:14]
    pick = np.concatenate([first, np.flatnonzero(~hit)[:28 - first.size]])
    assert pick.size == 28, f"n = {n}: {at.size} surface pixels"
    pos = np.concatenate([where[pick], rng.random((4, 2), dtype=f32)])
    ids = np.concatenate([frame_ids[at][pick], np.array((-1, n, 0, n - 1))]).astype(np.int32)
    return SimpleNamespace(path=c.path, w=cc.W, h=cc.H, lights=list(COUNT_LIGHTS), pos=np.ascontiguousarray(pos, f32),
                           ids=ids, n=n, gen=gen, turns=None, hitting=int(first.size))


def guards(sm, path, ids) -> dict:
    """The counts the main case is chosen for, from the oracle's own planes."""
    S = sm.c.shape[0]
    hits = (sm.c[..., 3] >= 0).sum(axis=0)
    m = resolve(sm, path, ids)[:, :3]
    asc = np.zeros_like(m)
    desc = np.zeros_like(m)
    for s in range(S):
        asc = asc + sm.c[s, :, :3]
        desc = desc + sm.c[S - 1 - s, :, :3]
    lit = (sm.classes == sc.LIT).any(axis=(0, 1))
    shadowed = (sm.classes == sc.SHADOWED).any(axis=(0, 1))
    return dict(no_surface=int((~sm.on).sum()), partial=int((sm.on & (hits > 0) & (hits < S)).sum()),
                full=int((sm.on & (hits == S)).sum()), lit=int((sm.on & lit).sum()), shadowed=int((sm.on & shadowed).sum()),
                mean_differs=int((sm.on & (m != sm.c[0, :, :3]).any(axis=1)).sum()),
                order_bits=int((asc.view(np.uint32) != desc.view(np.uint32)).sum()))
