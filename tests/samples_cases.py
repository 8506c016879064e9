"""Shared cases of the multi-sample tests (test_samples_host.py, test_gpu_samples.py): scene S, the
sample offsets, the oracle's per-sample frames and the numpy restatement of the resolve. Not a test
module.

Scene S is scene Q's geometry (tests/query_cases.py) with a random albedo per triangle and a
background that is not black: under Q's own flat albedo and zero background a resolve that drops
its misses or mixes up its rows would go unseen.

Expected values (DESIGN.md section 2 "Resolve") come from S per-sample RGBA frames -- the oracle's,
or srtTraceAsync's -- never from the resolve under test: float32, acc = c_0 then acc + c_s in
ascending s, rgb = acc / float32(S), alpha = float32(hits) / float32(S); compared on the uint32 view.
"""
from __future__ import annotations

import functools

import numpy as np

import query_cases as qc
from oracle import srt_oracle as oracle
from scenefile import read_scene, write_custom_scene

BACKGROUND = (0.1, 0.2, 0.3)
SHADE_TOL = 1e-5  # the project's shading tolerance against the oracle
INT_MAX, INT_MIN = 2**31 - 1, -2**31
BAND = (40, 78)  # rows 40..117: not tile-aligned


def write_scene_s(path):
    """Scene S: Q's vertices and camera, albedo U[0.2, 1]^3 per triangle (seed 21), background
    (0.1, 0.2, 0.3)."""
    cam, _, v, _ = read_scene(qc.write_scene_q(str(path) + ".q"))
    albedo = np.random.default_rng(21).uniform(0.2, 1.0, (len(v), 3)).astype(np.float32)
    return write_custom_scene(path, v, albedo=albedo, eye=cam[0:3], lookat=cam[3:6], up=cam[6:9], vfov=cam[9],
                              background=BACKGROUND)


def offsets(width: int, height: int, samples: int) -> np.ndarray:
    """(S, H, W, 2): sample s's offsets are query_cases.random_offsets(W, H, 100 + s)."""
    return np.stack([qc.random_offsets(width, height, 100 + s) for s in range(samples)])


def tolerance(samples: int) -> float:
    """Against the oracle: its shading tolerance plus the S - 1 adds and one division, each within
    2^-24 of values <= 1."""
    return SHADE_TOL + samples * 2.0 ** -24


def out_of_range_ids(n: int) -> np.ndarray:
    return np.array([-1, -5, n, n + 7, INT_MAX, INT_MIN], np.int64).astype(np.int32)


def expected(frames: np.ndarray, hit: np.ndarray | None = None) -> np.ndarray:
    """The resolve of S per-sample RGBA frames (S, rows, W, 4), restated in numpy. hit (S, rows, W):
    which samples hit; by default the frames' alpha (an id, -1 for a miss) says so."""
    f = np.asarray(frames, np.float32)
    samples = f.shape[0]
    if hit is None:
        hit = f[..., 3] >= 0
    acc = f[0, ..., :3].copy()
    for s in range(1, samples):
        acc = acc + f[s, ..., :3]
        assert acc.dtype == np.float32
    out = np.empty(f.shape[1:], np.float32)
    out[..., :3] = acc / np.float32(samples)
    out[..., 3] = np.asarray(hit).sum(axis=0).astype(np.float32) / np.float32(samples)
    return out


def assert_conditions(ids: np.ndarray, n: int, large_ids=qc.LARGE_IDS):
    """The sample ids (S, H, W) cover what the tests rely on: hits and misses, pixels of partial
    coverage, large-list winners."""
    samples = ids.shape[0]
    hit = (ids >= 0) & (ids < n)
    assert hit.mean() >= 0.10 and (~hit).mean() >= 0.10
    hits = hit.sum(axis=0)
    assert ((hits > 0) & (hits < samples)).mean() >= 0.02
    assert np.isin(ids, large_ids).mean() >= 0.01


def same_bits(name, got, want):
    g = np.ascontiguousarray(got, np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert g.shape == w.shape, f"{name}: shape {g.shape} != {w.shape}"
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, (f"{name}: {bad.size} values differ, first at {bad[0]}: "
                           f"{g.reshape(-1)[bad[0]]:#x} != {w.reshape(-1)[bad[0]]:#x}")


def check_against_oracle(name, got, frames) -> float:
    """Coverage exact, rgb within tolerance(S) of expected(the oracle's frames); the largest rgb
    difference."""
    want = expected(frames)
    same_bits(f"{name}: coverage", got[..., 3], want[..., 3])
    err = float(np.abs(got[..., :3].astype(np.float64) - want[..., :3].astype(np.float64)).max())
    print(f"{name}: max |rgb - oracle| = {err:.3e} (tolerance {tolerance(frames.shape[0]):.3e})")
    assert err <= tolerance(frames.shape[0]), f"{name}: rgb off by {err:.3e}"
    return err


def scatter_misses(ids: np.ndarray, n: int, count: int = 50, seed: int = 8):
    """A copy of the sample ids (S, H, W) with the out-of-range ids written over `count` samples
    that hit, and the flat indices of those samples."""
    out = np.array(ids, np.int32)
    flat = out.reshape(-1)
    hits = np.flatnonzero((flat >= 0) & (flat < n))
    at = np.random.default_rng(seed).choice(hits, count, replace=False)
    flat[at] = np.resize(out_of_range_ids(n), count)
    return out, at


def frames_with_misses(frames: np.ndarray, at: np.ndarray, background) -> np.ndarray:
    """The per-sample frames with the samples `at` (flat indices into (S, H, W)) turned into misses."""
    f = np.array(frames, np.float32)
    f.reshape(-1, 4)[at] = np.float32([*background, -1.0])
    return f


@functools.lru_cache(maxsize=None)
def oracle_frames(path: str, width: int, height: int, samples: int):
    """(offsets (S, H, W, 2), frames (S, H, W, 4), ids (S, H, W) int32, n): the oracle's frame of
    every sample, once per session, read-only. The ids are the frames' alpha channel."""
    off = offsets(width, height, samples)
    sc = oracle.OracleScene(path)
    frames = np.stack([sc.render(width, height, off[s]) for s in range(samples)])
    n = sc.n
    sc.close()
    ids = frames[..., 3].astype(np.int32)
    assert np.array_equal(ids.astype(np.float32), frames[..., 3])
    for a in (off, frames, ids):
        a.setflags(write=False)
    return off, frames, ids, n
