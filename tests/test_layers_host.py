"""Depth layers on the host (include/srt_layers.h): rtkLayersHost against the oracle's peeled
closest hits, rtkCompositeHost against the numpy restatement over the oracle's shades, the
argument errors and the exports. No GPU. Cases and expectations: tests/layers_cases.py."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import layers_cases as lc
import query_cases as qc
import simpleraytracer_amd.device as device
from simpleraytracer_amd import _native

REPO = Path(__file__).resolve().parents[1]
CASES = ("stack", "twins", "q")
EXPORTS = {"rtkLayersAsync", "rtkFrameAsync", "rtkCompositeAsync", "rtkLayersHost", "rtkCompositeHost"}


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("layers")
    return {name: lc.write_case(name, d / f"{name}.srt") for name in CASES}


@pytest.mark.parametrize("name", CASES)
def test_case_conditions(paths, name):
    for key in ("pixels", "mixed"):
        _, ids, t = lc.cached_layers(paths[name], name, key)
        lc.assert_conditions(name, ids, t)


@pytest.mark.parametrize("layers", [1, 2, 3, 8])
@pytest.mark.parametrize("name", CASES)
def test_host_layers_equal_the_oracle(paths, name, layers):
    w, h = lc.FRAMES[name]
    for key in ("pixels", "mixed"):
        pos, want_ids, want_t = lc.cached_layers(paths[name], name, key)
        ids, t = device.layers_host(paths[name], w, h, pos, layers)
        assert ids.shape == t.shape == (layers, len(pos))
        lc.assert_same(ids, t, want_ids[:layers], want_t[:layers])


@pytest.mark.parametrize("name", CASES)
def test_layer_0_is_the_point_query_and_layers_are_prefixes(paths, name):
    w, h = lc.FRAMES[name]
    pos, _, _ = lc.cached_layers(paths[name], name, "mixed")
    q_ids, q_t = device.query_host(paths[name], w, h, pos)
    prev = None
    for layers in range(1, lc.MAX_LAYERS + 1):
        ids, t = device.layers_host(paths[name], w, h, pos, layers)
        lc.assert_same(ids[0], t[0], q_ids, q_t)
        if prev is not None:
            lc.assert_same(ids[:-1], t[:-1], *prev)
        prev = (ids, t)


def test_out_of_range_and_nan_positions(paths):
    """Any float pair is a legal position: out-of-range ones get the brute-force answer (the mixed
    set holds them, compared with the oracle above), and a NaN position has no layers."""
    w, h = lc.FRAMES["stack"]
    pos, want_ids, _ = lc.cached_layers(paths["stack"], "stack", "mixed")
    outside = ~qc.in_range(pos)
    assert outside.sum() >= len(qc.OUT_OF_RANGE) ** 2
    nan = np.isnan(pos).any(axis=1)
    assert nan.sum() >= 13
    ids, t = device.layers_host(paths["stack"], w, h, pos, 8)
    assert np.all(ids[:, nan] == -1) and np.all(np.isposinf(t[:, nan]))
    assert np.all(want_ids[:, nan] == -1)


@pytest.fixture(scope="module")
def frame_case(paths):
    """The stack case's whole frame: offsets, the oracle's 8 id planes, their oracle shades, the
    opacity table. Read-only."""
    name = "stack"
    w, h = lc.FRAMES[name]
    off = lc.offsets(w, h)
    _, ids, _ = lc.cached_layers(paths[name], name, "pixels")
    ids = ids[:lc.MAX_LAYERS].reshape(lc.MAX_LAYERS, h, w)
    shaded = lc.shaded_layers(paths[name], w, h, ids, off)
    opa = lc.opacity(device.scene_triangles(paths[name]))
    for a in (off, shaded, opa):
        a.setflags(write=False)
    return paths[name], w, h, off, ids, shaded, opa


@pytest.mark.parametrize("layers", [1, 3, 8])
def test_host_composite_is_the_numpy_restatement(frame_case, layers):
    path, w, h, off, ids, shaded, opa = frame_case
    got = device.composite_host(path, w, h, off, ids[:layers], opa)
    want = lc.expected_composite(shaded[:layers], ids[:layers], opa, lc.BACKGROUND)
    print(f"composite_host K={layers}: max |got - want| = {np.abs(got - want).max():.3e}")
    lc.same_bits(f"composite_host K={layers}", got, want)


def test_host_composite_of_a_band(frame_case):
    path, w, h, off, ids, shaded, opa = frame_case
    r0, rows = lc.BANDS["stack"]
    got = device.composite_host(path, w, h, off[r0:r0 + rows], ids[:4, r0:r0 + rows], opa, row_begin=r0, row_count=rows)
    want = lc.expected_composite(shaded[:4, r0:r0 + rows], ids[:4, r0:r0 + rows], opa, lc.BACKGROUND)
    lc.same_bits("composite_host band", got, want)
    assert device.composite_host(path, w, h, off[:0], ids[:4, :0], opa, row_begin=h, row_count=0).shape == (0, w, 4)


def test_host_composite_opaque_is_the_shaded_frame_and_clear_is_the_background(frame_case):
    path, w, h, off, ids, shaded, opa = frame_case
    hit = ids[0] >= 0
    assert hit.any() and (~hit).any()
    ones = np.ones_like(opa)
    got = device.composite_host(path, w, h, off, ids, ones)
    lc.same_bits("opaque rgb", got[..., :3], shaded[0, ..., :3])
    assert np.array_equal(got[..., 3], hit.astype(np.float32))
    got = device.composite_host(path, w, h, off, ids, np.zeros_like(opa))
    want = np.broadcast_to(np.float32(lc.BACKGROUND + (0.0,)), (h, w, 4))
    lc.same_bits("clear", got, want)


def test_host_composite_stops_at_the_first_id_outside_the_scene(frame_case):
    """Ids outside [0, n) end a pixel's composite; a NaN opacity propagates."""
    path, w, h, off, ids, shaded, opa = frame_case
    n = len(opa)
    mixed = ids[:4].copy()
    bad = np.array([-1, -5, n, n + 7, 2**31 - 1, -2**31], np.int64).astype(np.int32)
    mixed[1].reshape(-1)[::7] = np.resize(bad, mixed[1].reshape(-1)[::7].size)
    got = device.composite_host(path, w, h, off, mixed, opa)
    lc.same_bits("stops", got, lc.expected_composite(shaded[:4], mixed, opa, lc.BACKGROUND))
    nan_opa = opa.copy()
    nan_opa[ids[0][ids[0] >= 0][0]] = np.nan
    got = device.composite_host(path, w, h, off, ids[:4], nan_opa)
    want = lc.expected_composite(shaded[:4], ids[:4], nan_opa, lc.BACKGROUND)
    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    lc.same_bits("nan opacity elsewhere", got[keep], want[keep])


def test_argument_errors(paths):
    L = _native.lib()
    path = str(paths["stack"]).encode()
    pos = (ctypes.c_float * 2)(0.5, 0.5)
    ids, t = (ctypes.c_int * 8)(), (ctypes.c_float * 8)()
    for layers in (0, 9):
        assert L.rtkLayersHost(path, 8, 8, pos, 1, layers, ids, t) == -1
        assert re.search(r"layers must be 1 to 8, got %d" % layers, _native.last_error())
    assert L.rtkLayersHost(None, 8, 8, pos, 1, 1, ids, t) == -1 and "scene_path" in _native.last_error()
    assert L.rtkLayersHost(path, 0, 8, pos, 1, 1, ids, t) == -1 and "width" in _native.last_error()
    assert L.rtkLayersHost(path, 8, 8, None, 1, 1, ids, t) == -1 and "positions" in _native.last_error()
    assert L.rtkLayersHost(path, 8, 8, pos, 1, 1, None, t) == -1 and "ids" in _native.last_error()
    assert L.rtkLayersHost(b"/nonexistent/scene.srt", 8, 8, pos, 1, 1, ids, t) == -1 and _native.last_error()
    assert L.rtkLayersHost(path, 8, 8, None, 0, 1, None, None) == 0
    assert L.rtkLayersHost(path, 8, 8, pos, 1, 8, ids, None) == 0  # t is optional
    off = (ctypes.c_float * 128)()
    cid = (ctypes.c_int * 64)()
    n = device.scene_triangles(paths["stack"])
    opa = (ctypes.c_float * n)()
    rgba = (ctypes.c_float * 256)()
    assert L.rtkCompositeHost(path, 8, 8, off, cid, 1, opa, 0, 8, rgba) == 0
    for layers in (0, 9):
        assert L.rtkCompositeHost(path, 8, 8, off, cid, layers, opa, 0, 8, rgba) == -1
        assert "layers must be 1 to 8" in _native.last_error()
    assert L.rtkCompositeHost(path, 8, 8, off, cid, 1, opa, 4, 5, rgba) == -1
    assert "row band outside the frame" in _native.last_error()
    for k, name in enumerate(("offsets", "ids", "opacity", "rgba")):
        args = [off, cid, opa, rgba]
        args[k] = None
        assert L.rtkCompositeHost(path, 8, 8, args[0], args[1], 1, args[2], 0, 8, args[3]) == -1
        assert name in _native.last_error()
    assert L.rtkCompositeHost(path, 8, 8, None, None, 1, None, 8, 0, None) == 0
    with pytest.raises(ValueError):
        device.layers_host(paths["stack"], 8, 8, np.zeros((3, 3), np.float32), 2)
    with pytest.raises(ValueError):
        device.layers_host(paths["stack"], 8, 8, np.zeros((3, 2), np.float32), 9)
    with pytest.raises(ValueError):
        device.composite_host(paths["stack"], 8, 8, np.zeros((8, 8, 2)), np.zeros((1, 8, 8)), np.zeros(n + 1))


def test_layer_exports_and_the_pinned_families():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("rtk")} == EXPORTS
    header = (REPO / "include" / "srt_layers.h").read_text()
    assert "ML_API" + "_ENTRY" not in header
    assert set(re.findall(r"RTK_API\s+int\s+(\w+)\s*\(", header)) == EXPORTS
    assert re.search(r"#define\s+RTK_MAX_LAYERS\s+8\b", header) and _native.RTK_MAX_LAYERS == lc.MAX_LAYERS == 8
    # the other families are unchanged: 14 ml* + 38 srt*, 3 rtq*, 3 rtg*, 3 rts*, 4 rtl*
    assert len({s for s in exported if s.startswith(("ml", "srt"))}) == 52
    for prefix, count in (("rtq", 3), ("rtg", 3), ("rts", 3), ("rtl", 4)):
        assert len({s for s in exported if s.startswith(prefix)}) == count
