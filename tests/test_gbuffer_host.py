"""G-buffer outputs on the host (include/srt_gbuffer.h): rtgPointsHost / device.attributes_host
against values from the oracle and numpy (tests/gbuffer_cases.py), the miss values, the argument
errors and the exports. No GPU."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gbuffer_cases as gc
import query_cases as qc
import simpleraytracer_amd.device as device
from simpleraytracer_amd import _native

REPO = Path(__file__).resolve().parents[1]
RTG = {"rtgFrameAsync", "rtgPointsAsync", "rtgPointsHost"}


@pytest.fixture(scope="module")
def scene_q(tmp_path_factory):
    return qc.write_scene_q(tmp_path_factory.mktemp("gbuffer") / "q.srt")


def test_host_attributes_on_q(scene_q):
    """Pixel positions and the mixed family, ids from rtqQueryHost: every plane against the oracle."""
    for key in ("pixels", "mixed"):
        pos, want_ids, exp = gc.cached_expected(scene_q, qc.W, qc.H, key)
        qc.assert_mix(want_ids)
        ids, t = device.query_host(scene_q, qc.W, qc.H, pos)
        assert np.array_equal(ids, want_ids)
        depth, bary, normal, albedo = device.attributes_host(scene_q, qc.W, qc.H, pos, ids)
        gc.check_planes(exp, depth, bary, normal, albedo)
        gc.check_misses(ids, exp.n, exp.background, depth, bary, normal, albedo)
        assert np.array_equal(depth.view(np.uint32), t.view(np.uint32))  # the query's own t
        if key == "pixels":
            # both branches of the normal's sign are exercised, and no cosine is near zero
            hit = exp.valid
            assert (exp.cos64[hit] > 0).sum() >= 1000 and (exp.cos64[hit] < 0).sum() >= 1000
            assert np.abs(exp.cos64[hit]).min() > 1e-3
            gc.check_shade(scene_q, qc.W, qc.H, qc.random_offsets(qc.W, qc.H, 3), ids, normal, albedo)


@pytest.mark.parametrize("name", ["cornell", "triangle"])
def test_host_attributes_on_builtin_scenes(scenes, name):
    off = qc.random_offsets(qc.W, qc.H, 3)
    pixels = device.pixel_positions(qc.W, qc.H, off)
    pos = np.concatenate([pixels[::3], qc.mixed_positions(qc.W, qc.H)])  # (a third of the pixels: the oracle's time)
    ids, t = device.query_host(scenes[name], qc.W, qc.H, pos)
    assert (ids >= 0).any() and (ids < 0).any()
    exp = gc.expected(scenes[name], qc.W, qc.H, pos, ids)
    depth, bary, normal, albedo = device.attributes_host(scenes[name], qc.W, qc.H, pos, ids)
    gc.check_planes(exp, depth, bary, normal, albedo)
    gc.check_misses(ids, exp.n, exp.background, depth, bary, normal, albedo)
    assert np.array_equal(depth.view(np.uint32), t.view(np.uint32))
    # the whole pixel grid against oracle.shade
    ids, _ = device.query_host(scenes[name], qc.W, qc.H, pixels)
    _, _, normal, albedo = device.attributes_host(scenes[name], qc.W, qc.H, pixels, ids)
    gc.check_shade(scenes[name], qc.W, qc.H, off, ids, normal, albedo)


def test_host_miss_values(scene_q):
    """Ids outside the scene, at ordinary, NaN and out-of-range positions: the miss values."""
    _, _, exp = gc.cached_expected(scene_q, qc.W, qc.H, "mixed")
    bad = gc.miss_ids(exp.n)
    rng = np.random.default_rng(2)
    oor = qc.out_of_range_positions(rng)
    pos = np.concatenate([rng.random((len(bad), 2), dtype=np.float32), oor])
    ids = np.concatenate([bad, np.full(len(oor), -1, np.int32)])
    assert np.isnan(pos).any() and np.isinf(pos).any()
    depth, bary, normal, albedo = device.attributes_host(scene_q, qc.W, qc.H, pos, ids)
    gc.check_misses(ids, exp.n, exp.background, depth, bary, normal, albedo)
    assert np.all(np.isposinf(depth)) and np.all(albedo[:, 3] == -1.0)


def test_host_miss_background(tmp_path):
    """A miss's albedo is the scene's background."""
    from scenefile import write_custom_scene

    path = write_custom_scene(tmp_path / "bg.srt", np.float32([[0, 0, 3, 1, 0, 3, 0, 1, 3]]),
                              background=(0.25, 0.5, 0.75))
    pos = np.float32([[0.5, 0.5], [0.01, 0.01]])
    _, _, normal, albedo = device.attributes_host(path, 64, 64, pos, np.int32([-1, 1]))
    assert np.array_equal(albedo, np.float32([[0.25, 0.5, 0.75, -1.0]] * 2))
    assert np.array_equal(normal, np.float32([[0, 0, 0, 1]] * 2))


def test_host_errors(scene_q):
    L = _native.lib()
    path = str(scene_q).encode()
    pos = (ctypes.c_float * 2)(0.5, 0.5)
    ids = (ctypes.c_int * 1)(0)
    depth = (ctypes.c_float * 1)(-5.0)
    out = _native.RtgOutputs(ctypes.sizeof(_native.RtgOutputs), ctypes.addressof(depth), 0, 0, 0)
    assert ctypes.sizeof(_native.RtgOutputs) == 40
    assert L.rtgPointsHost(path, 8, 8, pos, ids, 1, ctypes.byref(out)) == 0 and depth[0] != -5.0
    assert L.rtgPointsHost(None, 8, 8, pos, ids, 1, ctypes.byref(out)) == -1 and _native.last_error()
    assert L.rtgPointsHost(path, 0, 8, pos, ids, 1, ctypes.byref(out)) == -1
    assert L.rtgPointsHost(path, 8, 0, pos, ids, 1, ctypes.byref(out)) == -1
    assert L.rtgPointsHost(path, 8, 8, None, ids, 1, ctypes.byref(out)) == -1
    assert L.rtgPointsHost(path, 8, 8, pos, None, 1, ctypes.byref(out)) == -1
    assert L.rtgPointsHost(path, 8, 8, pos, ids, 1, None) == -1 and "outputs" in _native.last_error()
    assert L.rtgPointsHost(b"/nonexistent/scene.srt", 8, 8, pos, ids, 1, ctypes.byref(out)) == -1
    # struct_size is checked
    for size in (0, 32, 48):
        wrong = _native.RtgOutputs(size, ctypes.addressof(depth), 0, 0, 0)
        assert L.rtgPointsHost(path, 8, 8, pos, ids, 1, ctypes.byref(wrong)) == -1
        assert "struct_size" in _native.last_error()
    # count == 0 and all planes null: nothing to do, nothing read
    depth[0] = -5.0
    assert L.rtgPointsHost(path, 8, 8, None, None, 0, ctypes.byref(out)) == 0 and depth[0] == -5.0
    none = _native.RtgOutputs(ctypes.sizeof(_native.RtgOutputs), 0, 0, 0, 0)
    assert L.rtgPointsHost(path, 8, 8, None, None, 1, ctypes.byref(none)) == 0
    # the wrapper's shape checks
    with pytest.raises(ValueError):
        device.attributes_host(scene_q, 8, 8, np.zeros((3, 3), np.float32), np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        device.attributes_host(scene_q, 8, 8, np.zeros((3, 2), np.float32), np.zeros(4, np.int32))
    d, b, n, a = device.attributes_host(scene_q, 8, 8, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    assert d.shape == (0,) and b.shape == (0, 2) and n.shape == (0, 4) and a.shape == (0, 4)


def test_gbuffer_exports_and_the_pinned_families():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("rtg")} == RTG
    header = (REPO / "include" / "srt_gbuffer.h").read_text()
    assert "ML_API" + "_ENTRY" not in header
    assert set(re.findall(r"RTG_API\s+int\s+(\w+)\s*\(", header)) == RTG
    # the other families are unchanged: 14 ml* + 38 srt*, three rtq*
    assert len({s for s in exported if s.startswith(("ml", "srt"))}) == 52
    assert {s for s in exported if s.startswith("rtq")} == {"rtqQueryAsync", "rtqQueryHost", "rtqTileHost"}
    L = _native.lib()
    for name in RTG:
        assert getattr(L, name) is not None
