"""Point queries on the host (include/srt_query.h): rtqQueryHost against the oracle, the kernel's
tile lookup (rtqTileHost) against the analytic tile boxes, and the exports. No GPU."""
from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import query_cases as qc
import simpleraytracer_amd.device as device
from simpleraytracer_amd import _native

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def scene_q(tmp_path_factory):
    return qc.write_scene_q(tmp_path_factory.mktemp("query") / "q.srt")


def test_host_query_equals_oracle_on_q(scene_q):
    for key in ("pixels", "mixed"):
        pos, want_ids, want_t = qc.cached_answers(scene_q, qc.W, qc.H, key)
        qc.assert_mix(want_ids)
        ids, t = device.query_host(scene_q, qc.W, qc.H, pos)
        qc.assert_same(ids, t, want_ids, want_t)
        assert np.all(np.isposinf(t[ids < 0])) and np.all(np.isfinite(t[ids >= 0]))
    # the out-of-range family is in the mixed set, and a NaN position misses
    pos, want_ids, _ = qc.cached_answers(scene_q, qc.W, qc.H, "mixed")
    assert (~qc.in_range(pos)).sum() >= len(qc.OUT_OF_RANGE) ** 2
    assert np.all(want_ids[np.isnan(pos).any(axis=1)] == -1)


@pytest.mark.parametrize("name", ["cornell", "triangle"])
def test_host_query_equals_oracle_on_builtin_scenes(scenes, name):
    pos = np.concatenate([device.pixel_positions(qc.W, qc.H, qc.random_offsets(qc.W, qc.H, 3)),
                          qc.mixed_positions(qc.W, qc.H)])
    want_ids, want_t = qc.oracle_answers(scenes[name], qc.W, qc.H, pos)
    assert (want_ids >= 0).any()
    ids, t = device.query_host(scenes[name], qc.W, qc.H, pos)
    qc.assert_same(ids, t, want_ids, want_t)


def test_pixel_positions_are_the_oracles():
    off = qc.random_offsets(7, 5, 1)
    pos = device.pixel_positions(7, 5, off).reshape(5, 7, 2)
    for y in range(5):
        for x in range(7):
            fx, fy = qc.oracle.pixel_position(x, y, float(off[y, x, 0]), float(off[y, x, 1]), 7, 5)
            assert pos[y, x, 0] == np.float32(fx) and pos[y, x, 1] == np.float32(fy)


def test_host_query_errors(scene_q):
    L = _native.lib()
    ids, t = (ctypes.c_int * 1)(), (ctypes.c_float * 1)()
    pos = (ctypes.c_float * 2)(0.5, 0.5)
    assert L.rtqQueryHost(None, 8, 8, pos, 1, ids, t) == -1 and _native.last_error()
    assert L.rtqQueryHost(str(scene_q).encode(), 0, 8, pos, 1, ids, t) == -1
    assert L.rtqQueryHost(str(scene_q).encode(), 8, 8, None, 1, ids, t) == -1
    assert L.rtqQueryHost(b"/nonexistent/scene.srt", 8, 8, pos, 1, ids, t) == -1 and _native.last_error()
    assert L.rtqQueryHost(str(scene_q).encode(), 8, 8, None, 0, None, None) == 0
    with pytest.raises(ValueError):
        device.query_host(scene_q, 8, 8, np.zeros((3, 3), np.float32))


TILE_SHAPES = [(1, 1), (63, 15), (64, 16), (65, 17), (200, 150), (333, 170), (1920, 1080), (3840, 2160)]


@pytest.mark.parametrize("width,height", TILE_SHAPES)
def test_tile_lookup_returns_a_tile_whose_box_contains_the_position(width, height):
    L = _native.lib()
    rng = np.random.default_rng(width * 10007 + height)
    pos = np.concatenate([qc.boundary_positions(width, height, rng), qc.out_of_range_positions(rng),
                          rng.random((10000, 2), dtype=np.float32)])
    nx, ny = (width + 63) // 64, (height + 15) // 16
    col, row = ctypes.c_int(), ctypes.c_int()
    rc = np.empty(len(pos), np.int64)
    cols = np.zeros(len(pos), np.int64)
    rows = np.zeros(len(pos), np.int64)
    for k, (fx, fy) in enumerate(pos):
        rc[k] = L.rtqTileHost(width, height, fx, fy, ctypes.byref(col), ctypes.byref(row))
        if rc[k] == 0:
            cols[k], rows[k] = col.value, row.value
    inside = qc.in_range(pos)
    assert inside.sum() >= 10000 and (~inside).sum() >= len(qc.OUT_OF_RANGE) ** 2
    assert np.array_equal(rc == 0, inside) and np.array_equal(rc == -1, ~inside)
    c, r, p = cols[inside], rows[inside], pos[inside]
    assert c.min() >= 0 and c.max() < nx and r.min() >= 0 and r.max() < ny
    # the analytic box of the returned tile, in float32: [fl(64 c / W), fl((64 c + 64) / W)] x
    # [fl(16 r / H), fl((16 r + 16) / H)]
    wf, hf = np.float32(width), np.float32(height)
    xlo, xhi = (c * 64).astype(np.float32) / wf, (c * 64 + 64).astype(np.float32) / wf
    ylo, yhi = (r * 16).astype(np.float32) / hf, (r * 16 + 16).astype(np.float32) / hf
    assert xlo.dtype == np.float32 and yhi.dtype == np.float32
    assert np.all((xlo <= p[:, 0]) & (p[:, 0] <= xhi) & (ylo <= p[:, 1]) & (p[:, 1] <= yhi))
    # fx == 1.0 belongs to the last column, fy == 1.0 to the last row
    assert L.rtqTileHost(width, height, 1.0, 1.0, ctypes.byref(col), ctypes.byref(row)) == 0
    assert (col.value, row.value) == (nx - 1, ny - 1)
    assert device.tile_of(width, height, 0.0, 0.0) == (0, 0)
    assert device.tile_of(width, height, float("nan"), 0.5) is None


def test_query_exports_and_the_pinned_families():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"rtqQueryAsync", "rtqQueryHost", "rtqTileHost"} <= exported
    assert {s for s in exported if s.startswith("rtq")} == {"rtqQueryAsync", "rtqQueryHost", "rtqTileHost"}
    header = (REPO / "include" / "srt_query.h").read_text()
    assert "ML_API" + "_ENTRY" not in header
    assert set(re.findall(r"RTQ_API\s+int\s+(\w+)\s*\(", header)) == {"rtqQueryAsync", "rtqQueryHost", "rtqTileHost"}
    # the ml* and srt* families are unchanged: 14 + 38
    assert len({s for s in exported if s.startswith(("ml", "srt"))}) == 52
    L = _native.lib()
    for name in ("rtqQueryAsync", "rtqQueryHost", "rtqTileHost"):
        assert getattr(L, name) is not None
