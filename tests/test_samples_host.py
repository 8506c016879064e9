"""Multi-sample frames on the host (include/srt_samples.h): rtsResolveHost / device.resolve_host
against the numpy restatement of the resolve over the oracle's per-sample frames
(tests/samples_cases.py), the invariants, the argument errors, the exports and
samples.stratified_offsets. No GPU."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gbuffer_cases as gc
import query_cases as qc
import samples_cases as sc
import simpleraytracer_amd.device as device
from simpleraytracer_amd import _native
from simpleraytracer_amd.samples import grid_side, stratified_offsets

REPO = Path(__file__).resolve().parents[1]
RTS = {"rtsResolveAsync", "rtsRenderAsync", "rtsResolveHost"}
W, H, S = qc.W, qc.H, 5


@pytest.fixture(scope="module")
def scene_s(tmp_path_factory):
    return sc.write_scene_s(tmp_path_factory.mktemp("samples") / "s.srt")


@pytest.fixture(scope="module")
def resolved(scene_s):
    """resolve_host of the whole 200 x 150 frame, S = 5, from the oracle's ids: once, read-only."""
    off, frames, ids, n = sc.oracle_frames(scene_s, W, H, S)
    sc.assert_conditions(ids, n)
    out = device.resolve_host(scene_s, W, H, off, ids)
    out.setflags(write=False)
    return out


def sample_shade(path, w, h, off, ids):
    """The library's own shade of one sample plane, (H, W, 3): albedo.rgb * normal.w of the host
    G-buffer, which is the traced pixel bit for bit (tests/test_gbuffer_host.py)."""
    _, _, normal, albedo = device.attributes_host(path, w, h, device.pixel_positions(w, h, off), ids.reshape(-1))
    return gc.composed_rgba(normal, albedo).reshape(h, w, 4)[..., :3]


def test_resolve_host_against_the_oracle(scene_s, resolved):
    """Coverage exact; rgb within 1e-5 + 5 * 2^-24 = 1.03e-5 of the numpy resolve of the oracle's
    five frames. Observed: a largest difference of 0 (the host shade has the oracle's bits)."""
    off, frames, ids, n = sc.oracle_frames(scene_s, W, H, S)
    assert resolved.shape == (H, W, 4) and resolved.dtype == np.float32
    sc.check_against_oracle("resolve_host 200x150 S=5", resolved, frames)
    hits = (ids >= 0).sum(axis=0)
    assert np.array_equal(resolved[..., 3], hits.astype(np.float32) / np.float32(S))
    assert set(np.unique(resolved[..., 3])) == {np.float32(k) / np.float32(S) for k in range(S + 1)}


def test_resolve_host_is_the_numpy_resolve_of_its_own_samples(scene_s, resolved):
    """Bit-equal to expected() over the library's own per-sample shades: the order of the adds and
    the one division are the restatement's."""
    off, _, ids, n = sc.oracle_frames(scene_s, W, H, S)
    own = np.zeros((S, H, W, 4), np.float32)
    for s in range(S):
        own[s, ..., :3] = sample_shade(scene_s, W, H, off[s], ids[s])
    sc.same_bits("resolve_host", resolved, sc.expected(own, hit=ids >= 0))


def test_one_sample_and_equal_copies(scene_s):
    """S = 1, and the same plane two and four times: the per-sample shade, bit for bit."""
    off, _, ids, _ = sc.oracle_frames(scene_s, W, H, S)
    want = sample_shade(scene_s, W, H, off[2], ids[2])
    one = device.resolve_host(scene_s, W, H, [off[2]], [ids[2]])
    sc.same_bits("S = 1", one[..., :3], want)
    assert np.array_equal(one[..., 3], (ids[2] >= 0).astype(np.float32))
    for copies in (2, 4):
        again = device.resolve_host(scene_s, W, H, [off[2]] * copies, [ids[2]] * copies)
        sc.same_bits(f"{copies} copies", again, one)


def test_band(scene_s, resolved):
    off, _, ids, _ = sc.oracle_frames(scene_s, W, H, S)
    r0, rows = sc.BAND
    band = device.resolve_host(scene_s, W, H, off[:, r0:r0 + rows], ids[:, r0:r0 + rows], row_begin=r0, row_count=rows)
    sc.same_bits("band 40..117", band, resolved[r0:r0 + rows])
    assert device.resolve_host(scene_s, W, H, off[:, :0], ids[:, :0], row_begin=H, row_count=0).shape == (0, W, 4)


def test_out_of_range_ids(scene_s, resolved):
    """Ids outside the scene over 50 samples that hit: those samples are misses, every other
    pixel keeps its bits."""
    off, frames, ids, n = sc.oracle_frames(scene_s, W, H, S)
    mixed, at = sc.scatter_misses(ids, n)
    assert set(mixed.reshape(-1)[at]) == set(sc.out_of_range_ids(n))
    got = device.resolve_host(scene_s, W, H, off, mixed)
    sc.check_against_oracle("out-of-range ids", got, sc.frames_with_misses(frames, at, sc.BACKGROUND))
    touched = np.zeros(H * W, bool)
    touched[at % (H * W)] = True
    assert np.all(got.reshape(-1, 4)[touched, 3] < resolved.reshape(-1, 4)[touched, 3])
    sc.same_bits("the other pixels", got.reshape(-1, 4)[~touched], resolved.reshape(-1, 4)[~touched])


def test_host_errors(scene_s):
    L = _native.lib()
    path = str(scene_s).encode()
    w = h = 8
    off = np.full((h, w, 2), 0.5, np.float32)
    ids = np.full((h, w), -1, np.int32)
    rgba = np.full((h, w, 4), -5.0, np.float32)
    arr = ctypes.c_void_p * 2
    offs, idp = arr(off.ctypes.data, off.ctypes.data), arr(ids.ctypes.data, ids.ctypes.data)
    out = rgba.ctypes.data

    def call(p=path, ww=w, hh=h, o=offs, i=idp, s=2, r0=0, rows=h, dst=out):
        return L.rtsResolveHost(p, ww, hh, o, i, s, r0, rows, dst)

    assert call() == 0 and np.array_equal(rgba, np.tile(np.float32([*sc.BACKGROUND, 0.0]), (h, w, 1)))
    assert call(p=None) == -1 and "scene_path" in _native.last_error()
    assert call(ww=0) == -1 and call(hh=0) == -1
    assert call(s=0) == -1 and "samples" in _native.last_error()
    assert call(s=_native.RTS_MAX_SAMPLES + 1) == -1 and "samples" in _native.last_error()
    assert call(o=None) == -1 and "offsets is NULL" in _native.last_error()
    assert call(i=None) == -1 and "ids is NULL" in _native.last_error()
    assert call(o=arr(off.ctypes.data, None)) == -1 and "offsets[1]" in _native.last_error()
    assert call(i=arr(None, ids.ctypes.data)) == -1 and "ids[0]" in _native.last_error()
    assert call(dst=None) == -1 and "rgba" in _native.last_error()
    assert call(r0=1) == -1 and "outside the frame" in _native.last_error()
    assert call(r0=h + 1, rows=0) == -1 and "outside the frame" in _native.last_error()
    assert call(p=b"/nonexistent/scene.srt") == -1
    # no rows: nothing to do, nothing read
    rgba[:] = -5.0
    assert call(o=None, i=None, rows=0, dst=None) == 0 and call(r0=h, rows=0) == 0 and np.all(rgba == -5.0)
    # the wrapper's checks
    with pytest.raises(ValueError):
        device.resolve_host(scene_s, w, h, [off, off], [ids])
    with pytest.raises(ValueError):
        device.resolve_host(scene_s, w, h, [], [])
    with pytest.raises(ValueError):
        device.resolve_host(scene_s, w, h, [off] * 17, [ids] * 17)
    with pytest.raises(ValueError):
        device.resolve_host(scene_s, w, h, [off[:, :-1]], [ids])
    with pytest.raises(ValueError):
        device.resolve_host(scene_s, w, h, [off], [ids[:-1]])
    assert device.resolve_host(scene_s, w, h, [off] * 16, [ids] * 16).shape == (h, w, 4)


def test_samples_exports_and_the_pinned_families():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("rts")} == RTS
    header = (REPO / "include" / "srt_samples.h").read_text()
    assert "ML_API" + "_ENTRY" not in header
    assert set(re.findall(r"RTS_API\s+int\s+(\w+)\s*\(", header)) == RTS
    assert int(re.search(r"#define RTS_MAX_SAMPLES (\d+)", header).group(1)) == _native.RTS_MAX_SAMPLES == 16
    # the other families are unchanged: 14 ml* + 38 srt*, three rtq*, three rtg*
    assert len({s for s in exported if s.startswith(("ml", "srt"))}) == 52
    assert len({s for s in exported if s.startswith("rtq")}) == 3 and len({s for s in exported if s.startswith("rtg")}) == 3


@pytest.mark.parametrize("samples", [1, 2, 4, 5, 9, 16])
def test_stratified_offsets(samples):
    w, h = 37, 11
    off = stratified_offsets(w, h, samples, seed=4)
    assert off.shape == (samples, h, w, 2) and off.dtype == np.float32
    assert off.min() >= 0.0 and off.max() < 1.0
    g = grid_side(samples)
    assert g * g >= samples and (g - 1) * (g - 1) < samples
    cell = np.floor(off.astype(np.float64) * g).astype(np.int64)  # (exact: 24-bit values times a small integer)
    s = np.arange(samples)[:, None, None]
    assert np.array_equal(cell[..., 0], np.broadcast_to(s % g, (samples, h, w)))
    assert np.array_equal(cell[..., 1], np.broadcast_to(s // g, (samples, h, w)))
    assert np.array_equal(off, stratified_offsets(w, h, samples, seed=4))
    assert not np.array_equal(off, stratified_offsets(w, h, samples, seed=5))
    # jittered: a cell's values are not all alike
    assert np.unique(off[0, ..., 0]).size > w * h // 2
    with pytest.raises(ValueError):
        stratified_offsets(w, h, 0, seed=4)
