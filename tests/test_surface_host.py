"""Vertex attributes on the host (include/srt_surface.h): rtvSurfaceHost / rtvInterpolateHost against
the numpy float32 restatement of tests/surface_cases.py on the bits, the identities that tie the
family to the G-buffer's, the miss values, the derived tolerance of a flat normals table, the
argument errors and the exports. No GPU."""
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
import surface_cases as sv
from simpleraytracer_amd import _native
from simpleraytracer_amd.device import Surface

REPO = Path(__file__).resolve().parents[1]
RTV = {"rtvSurfaceFrameAsync", "rtvSurfacePointsAsync", "rtvInterpolateFrameAsync", "rtvInterpolatePointsAsync",
       "rtvSurfaceHost", "rtvInterpolateHost", "rtvObjAttributesHost"}
TABLE_SEED = 27  # (chosen so that every tap path below is taken often enough: test_tap_paths)
W, H = qc.W, qc.H


@pytest.fixture(scope="module")
def scene_q(tmp_path_factory):
    return qc.write_scene_q(tmp_path_factory.mktemp("surface") / "q.srt")


@pytest.fixture(scope="module")
def case_q(scene_q):
    """Scene Q's 'pixels' pairs, their E_k and det, and the random tables (planted uvs on six hit triangles)."""
    ev = sv.cached_edges(scene_q, W, H, "pixels")
    return ev, sv.tables(ev.n, TABLE_SEED, ev.ids)


def host(path, ev, surface):
    return device.surface_host(path, W, H, ev.pos, ev.ids, surface)


def test_specification_self_check(scene_q, scenes):
    """The restatement's interpolated hit point against eye + t d in float64 (surface_cases)."""
    sv.check_position_error(scene_q, W, H, "q")
    sv.check_position_error(scenes["cornell"], W, H, "cornell")


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_interpolation(scene_q, case_q, channels):
    ev, tb = case_q
    table = np.ascontiguousarray(tb.generic[:, :, :channels])
    got = device.interpolate_host(scene_q, W, H, ev.pos, ev.ids, table)
    assert got.shape == (len(ev.ids), channels)
    sv.same_bits("interpolation", got, sv.interpolate(ev, table))
    if channels == 4:  # channel c of a C = 4 call is the C = 1 call on that channel
        for c in range(4):
            one = device.interpolate_host(scene_q, W, H, ev.pos, ev.ids, np.ascontiguousarray(tb.generic[:, :, c:c + 1]))
            sv.same_bits(f"channel {c}", one[:, 0], got[:, c])


def test_weights_are_the_gbuffer_barycentrics(scene_q, case_q):
    """A table with corner 1 = 1 and the others 0 gives bary[:, 0], corner 2 bary[:, 1] (hit pairs)."""
    ev, _ = case_q
    _, bary, _, _ = device.attributes_host(scene_q, W, H, ev.pos, ev.ids)
    _, _, exp = gc.cached_expected(scene_q, W, H, "pixels")
    hit = ev.valid
    for corner in (1, 2):
        table = np.zeros((ev.n, 3, 1), np.float32)
        table[:, corner, 0] = 1.0
        got = device.interpolate_host(scene_q, W, H, ev.pos, ev.ids, table)[:, 0]
        sv.same_bits(f"corner {corner} against rtg", got[hit], bary[hit, corner - 1])
        sv.same_bits(f"corner {corner} against the oracle", got[hit], exp.bary[hit, corner - 1])


@pytest.mark.parametrize("size", sv.TEXTURE_SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_surface_planes(scene_q, case_q, size):
    """normal, uv, albedo and rgba on the bits: repeat and clamp, bilinear and nearest, modulate on and off."""
    ev, tb = case_q
    tex = sv.texture(*size, seed=5)
    for wrap in sv.WRAPS:
        for filt in sv.FILTERS:
            for modulate in (False, True):
                exp = sv.expected(ev, tb.normals, tb.uvs, tex, wrap, filt, modulate)
                got = host(scene_q, ev, Surface(tb.normals, tb.uvs, tex, wrap, filt, modulate))
                sv.check_surface(exp, *got)
    if size == (1, 1):  # a + s (a - a) = a: that texel on every hit
        _, albedo, _, _ = host(scene_q, ev, Surface(None, tb.uvs, tex))
        hit = ev.valid
        sv.same_bits("1 x 1 texture", albedo[hit, :3], np.tile(tex[0, 0, :3], (int(hit.sum()), 1)))


def test_tap_paths(case_q):
    """On the restatement alone: the planted uvs are hit, and at least 100 hit elements take each
    path of the bilinear taps -- i0 wrapped, i1 wrapped, neither -- on each axis."""
    ev, tb = case_q
    assert all((ev.ids == i).any() for i in tb.planted)
    uv = sv.interpolate(ev, tb.uvs)[ev.valid]
    assert np.isnan(uv).any() and (uv == 0).any() and (sv.wrap(uv[:, 0], False) == 1).any()
    for th, tw in ((3, 5), (64, 64)):
        for wrap in sv.WRAPS:
            exp = sv.expected(ev, None, tb.uvs, sv.texture(th, tw, 5), wrap, "bilinear")
            for axis, paths in zip("uv", exp.paths):
                counts = [int((paths == k).sum()) for k in range(3)]
                assert min(counts) >= 100, f"{tw} x {th}, {wrap}, {axis}: (none, i0, i1) = {counts}"


def test_optional_inputs_fall_back_to_the_gbuffer(scene_q, case_q):
    """No normals and no texture: rtgPointsHost's normal and albedo planes, rgba = albedo.rgb * normal.w."""
    ev, tb = case_q
    _, _, g_normal, g_albedo = device.attributes_host(scene_q, W, H, ev.pos, ev.ids)
    for surface in (Surface(), Surface(uvs=tb.uvs)):
        normal, albedo, rgba, uv = host(scene_q, ev, surface)
        sv.same_bits("normal", normal, g_normal)
        sv.same_bits("albedo", albedo, g_albedo)
        sv.same_bits("rgba", rgba, gc.composed_rgba(g_normal, g_albedo))
        sv.same_bits("uv", uv, sv.expected(ev, None, surface.uvs).uv)
    # each of the two alone: the other plane keeps its fallback
    tex = sv.texture(3, 5, 5)
    normal, albedo, rgba, _ = host(scene_q, ev, Surface(tb.normals))
    sv.same_bits("albedo without a texture", albedo, g_albedo)
    sv.same_bits("rgba", rgba, gc.composed_rgba(normal, albedo))
    normal, albedo, rgba, _ = host(scene_q, ev, Surface(None, tb.uvs, tex))
    sv.same_bits("normal without normals", normal, g_normal)
    sv.same_bits("albedo", albedo, sv.expected(ev, None, tb.uvs, tex).albedo)
    sv.same_bits("rgba", rgba, gc.composed_rgba(normal, albedo))


def test_miss_values(scene_q, case_q):
    """Ids outside the scene, at ordinary, NaN and out-of-range positions: the miss values."""
    ev, tb = case_q
    bad = gc.miss_ids(ev.n)
    rng = np.random.default_rng(2)
    oor = qc.out_of_range_positions(rng)
    pos = np.concatenate([rng.random((len(bad), 2), dtype=np.float32), oor])
    ids = np.concatenate([bad, np.full(len(oor), -1, np.int32)])
    tex = sv.texture(3, 5, 5)
    for surface in (Surface(), Surface(tb.normals, tb.uvs, tex, modulate=True)):
        got = device.surface_host(scene_q, W, H, pos, ids, surface)
        for name, g, want in zip(("normal", "albedo", "rgba", "uv"), got, sv.miss_planes(len(ids), ev.background)):
            sv.same_bits(f"miss {name}", g, want)
    out = device.interpolate_host(scene_q, W, H, pos, ids, tb.generic)
    sv.same_bits("miss interpolation", out, np.zeros((len(ids), 4), np.float32))


def test_flat_normals_give_the_geometric_normal(scene_q, case_q):
    """Corner normals all equal to the triangle's float32 N: the unit normal within 2^-20 per
    component of rtg's -- positive weights, so no cancellation: at most about 5 * 2^-24 relative
    from the weights, products and sums, 3 * 2^-24 from the normalisation, a margin of 2 -- and the
    cosine within 1e-5 of rtg's .w."""
    ev, _ = case_q
    v = ev.vertices.reshape(-1, 3, 3)
    n32 = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert n32.dtype == np.float32
    flat = np.repeat(n32[:, None, :], 3, axis=1)
    _, _, g_normal, _ = device.attributes_host(scene_q, W, H, ev.pos, ev.ids)
    normal, _, _, _ = host(scene_q, ev, Surface(flat))
    hit = ev.valid
    assert float(np.abs(normal[hit, :3] - g_normal[hit, :3]).max()) <= 2.0 ** -20
    assert float(np.abs(normal[hit, 3] - g_normal[hit, 3]).max()) <= 1e-5
    sv.same_bits("miss normal", normal[~hit], g_normal[~hit])


def test_host_errors(scene_q, case_q):
    ev, tb = case_q
    L = _native.lib()
    path = str(scene_q).encode()
    pos = (ctypes.c_float * 2)(0.5, 0.5)
    ids = (ctypes.c_int * 1)(0)
    plane = (ctypes.c_float * 4)(-5.0, -5.0, -5.0, -5.0)
    uvs = np.zeros((ev.n, 3, 2), np.float32)
    tex = np.zeros((2, 2, 4), np.float32)
    size_s, size_o = ctypes.sizeof(_native.RtvSurface), ctypes.sizeof(_native.RtvOutputs)
    assert (size_s, size_o) == (56, 40)
    s = _native.RtvSurface(size_s, 0, 0, 0, 0, 0, 0)
    out = _native.RtvOutputs(size_o, 0, 0, ctypes.addressof(plane), 0)

    def call(surface=s, outputs=out, p=path, w=8, h=8, positions=pos, idv=ids, count=1):
        return L.rtvSurfaceHost(p, w, h, positions, idv, count, ctypes.byref(surface) if surface else None,
                                ctypes.byref(outputs) if outputs else None)

    assert call() == 0 and plane[0] != -5.0
    assert call(p=None) == -1 and _native.last_error()
    assert call(w=0) == -1 and call(h=0) == -1
    assert call(positions=None) == -1 and "positions" in _native.last_error()
    assert call(idv=None) == -1 and "ids" in _native.last_error()
    assert call(surface=None) == -1 and "surface" in _native.last_error()
    assert call(outputs=None) == -1 and "outputs" in _native.last_error()
    assert call(p=b"/nonexistent/scene.srt") == -1
    for size in (0, 48, 64):
        assert call(surface=_native.RtvSurface(size, 0, 0, 0, 0, 0, 0)) == -1
        assert "rtv_surface.struct_size" in _native.last_error()
    for size in (0, 32, 48):
        assert call(outputs=_native.RtvOutputs(size, 0, 0, ctypes.addressof(plane), 0)) == -1
        assert "rtv_outputs.struct_size" in _native.last_error()
    for flags in (8, 16, 0x80000000 | 1):
        assert call(surface=_native.RtvSurface(size_s, 0, 0, 0, 0, 0, flags)) == -1
        assert "rtv_surface.flags" in _native.last_error()
    # a texture without uvs; a texture size outside the limits
    assert call(surface=_native.RtvSurface(size_s, 0, 0, tex.ctypes.data, 2, 2, 0)) == -1
    assert "rtv_surface.uvs" in _native.last_error()
    for tw, th, field in ((0, 2, "tex_width"), (16385, 2, "tex_width"), (2, 0, "tex_height"), (2, 16385, "tex_height")):
        assert call(surface=_native.RtvSurface(size_s, 0, uvs.ctypes.data, tex.ctypes.data, tw, th, 0)) == -1
        assert f"rtv_surface.{field}" in _native.last_error()
    assert call(surface=_native.RtvSurface(size_s, 0, uvs.ctypes.data, tex.ctypes.data, 2, 2, 7)) == 0
    # count == 0 and all planes null: nothing to do, nothing read
    plane[0] = -5.0
    assert call(positions=None, idv=None, count=0) == 0 and plane[0] == -5.0
    assert call(outputs=_native.RtvOutputs(size_o, 0, 0, 0, 0), positions=None, idv=None) == 0
    # the interpolation: channels outside 1..4, NULL inputs
    table = np.zeros((ev.n, 3, 4), np.float32)
    res = (ctypes.c_float * 4)()
    for channels in (0, 5):
        assert L.rtvInterpolateHost(path, 8, 8, pos, ids, 1, table.ctypes.data, channels, res) == -1
        assert "channels" in _native.last_error()
    assert L.rtvInterpolateHost(path, 8, 8, pos, ids, 1, table.ctypes.data, 4, res) == 0
    assert L.rtvInterpolateHost(path, 8, 8, pos, ids, 1, None, 4, res) == -1 and "table" in _native.last_error()
    assert L.rtvInterpolateHost(path, 8, 8, pos, ids, 1, table.ctypes.data, 4, None) == -1 and "out" in _native.last_error()
    assert L.rtvInterpolateHost(path, 8, 8, None, ids, 1, table.ctypes.data, 4, res) == -1
    assert L.rtvInterpolateHost(path, 8, 8, None, None, 0, None, 4, None) == 0
    assert L.rtvInterpolateHost(None, 8, 8, pos, ids, 1, table.ctypes.data, 4, res) == -1
    # the wrapper's checks
    with pytest.raises(ValueError):
        Surface(texture=tex)
    with pytest.raises(ValueError):
        Surface(wrap="mirror")
    with pytest.raises(ValueError):
        Surface(filter="cubic")
    with pytest.raises(ValueError):
        device.surface_host(scene_q, 8, 8, np.zeros((3, 3), np.float32), np.zeros(3, np.int32), Surface())
    with pytest.raises(ValueError):
        device.surface_host(scene_q, 8, 8, np.zeros((3, 2), np.float32), np.zeros(4, np.int32), Surface())
    with pytest.raises(ValueError):
        device.surface_host(scene_q, 8, 8, np.zeros((3, 2), np.float32), np.zeros(3, np.int32), Surface(tb.normals[:-1]))
    with pytest.raises(ValueError):
        device.surface_host(scene_q, 8, 8, np.zeros((3, 2), np.float32), np.zeros(3, np.int32),
                            Surface(uvs=tb.uvs, texture=np.zeros((2, 2, 3), np.float32)))
    with pytest.raises(ValueError):
        device.interpolate_host(scene_q, 8, 8, np.zeros((3, 2), np.float32), np.zeros(3, np.int32),
                                np.zeros((ev.n, 3, 5), np.float32))
    planes = device.surface_host(scene_q, 8, 8, np.zeros((0, 2), np.float32), np.zeros(0, np.int32), Surface())
    assert [p.shape for p in planes] == [(0, 4), (0, 4), (0, 4), (0, 2)]


def test_surface_exports_and_the_pinned_families():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("rtv")} == RTV
    header = (REPO / "include" / "srt_surface.h").read_text()
    assert "ML_API" + "_ENTRY" not in header
    assert set(re.findall(r"RTV_API\s+int\s+(\w+)\s*\(", header)) == RTV
    assert len({s for s in exported if s.startswith(("ml", "srt"))}) == 52  # 14 ml* + 38 srt*: unchanged
    L = _native.lib()
    for name in RTV:
        assert getattr(L, name) is not None
