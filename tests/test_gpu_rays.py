"""Ray queries on the device (include/srt_rays.h rtrClosestAsync, rtrOccludedAsync; rays.hip): the
closest hit and the occlusion of caller-supplied rays, answered from the scene's world-space tree.

Every comparison is exact -- ids equal, t and the barycentrics equal on the uint32 view, the
occlusion bytes equal -- against the host path (rtrClosestHost: brute force in ascending id, no
tree), which tests/test_rays_host.py ties to a numpy restatement of DESIGN.md section 2 "Rays".
Scenes and ray families are tests/rays_cases.py's; every test asserts its mix first.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import query_cases as qc
import rays_cases as rc
from scenefile import write_custom_scene

pytestmark = pytest.mark.gpu
f32 = np.float32


class Rig:
    """One scene on cuda:0; closest() and occluded() return numpy arrays."""

    def __init__(self, path):
        import torch

        import simpleraytracer_amd as srt

        self.torch = torch
        self.scene = srt.DeviceScene(path, 0)
        self.stream = torch.cuda.current_stream()

    def closest(self, rays, bary=True, stream=None):
        torch = self.torch
        n = len(rays)
        r = torch.from_numpy(np.array(rays, f32).reshape(n, 8)).cuda()  # (a copy: the shared cases are read-only)
        ids = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        t = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        b = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda") if bary else None
        torch.cuda.synchronize()
        self.scene.closest(r, ids, t, b, stream=self.stream if stream is None else stream)
        torch.cuda.synchronize()
        return ids.cpu().numpy(), t.cpu().numpy(), b.cpu().numpy() if bary else None

    def occluded(self, rays, stream=None):
        torch = self.torch
        n = len(rays)
        r = torch.from_numpy(np.array(rays, f32).reshape(n, 8)).cuda()
        out = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.scene.occluded(r, out, stream=self.stream if stream is None else stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def stats(self, capfd):
        lines = re.findall(r"srt rays: scene \S+ builds (\d+) allocations (\d+)", capfd.readouterr().err)
        assert lines, "no ray counters on stderr: is SRT_SETUP_LOG honoured?"
        return tuple(int(v) for v in lines[-1])

    def close(self):
        self.scene.close()


def default_env(monkeypatch):
    monkeypatch.delenv("SRT_RAYS", raising=False)


def check_scene(path, total, large_ids=None, monkeypatch=None):
    rays, ids, t, bary, occ = rc.host_answers(path, total)
    rc.assert_mix(ids, large_ids)
    rig = Rig(path)
    got = rig.closest(rays)
    got_occ = rig.occluded(rays)
    brute = brute_occ = None
    if monkeypatch is not None:
        monkeypatch.setenv("SRT_RAYS", "brute")
        brute = rig.closest(rays)
        brute_occ = rig.occluded(rays)
        monkeypatch.delenv("SRT_RAYS")
    rig.close()
    rc.assert_same(got, (ids, t, bary))
    assert np.array_equal(got_occ, occ)
    if brute is not None:
        rc.assert_same(brute, (ids, t, bary))
        assert np.array_equal(brute_occ, occ)
    return len(rays)


@pytest.mark.parametrize("name", ["q", "cornell", "soup2k"])
def test_device_equals_the_host(gpu, scenes, monkeypatch, name):
    """T2: about 4 000 mixed rays on Q, Cornell and soup2k: the tree's answers and the brute-force
    kernel's (SRT_RAYS=brute) are the host's."""
    default_env(monkeypatch)
    path = rc.q_path() if name == "q" else scenes[name]
    count = check_scene(path, 2500, qc.LARGE_IDS if name == "q" else None, monkeypatch)
    assert 3500 <= count <= 4500


@pytest.mark.parametrize("n", rc.COUNT_SOUPS)
def test_triangle_counts_where_the_tree_changes_shape(gpu, monkeypatch, n):
    """T2: 512 rays on soups of 0, 1, 7, 8, 9, 63, 64, 65, 512, 513 and 4 097 triangles: a partial
    last leaf, a partial last node, one more level."""
    default_env(monkeypatch)
    path = rc.soup_path(n)
    if n == 0:
        # No loader gives a scene without triangles (a file of 0 triangles is refused, as is an OBJ
        # without faces), so the library's "n == 0 stores misses" path cannot be reached through
        # the public interface: the case is the refusal, and the host path's misses on no triangles
        # are test_rays_host's numpy_answers' n == 0 branch.
        import simpleraytracer_amd as srt

        with pytest.raises(srt.SrtError, match="bad triangle count 0"):
            srt.DeviceScene(path, 0)
        return
    count = check_scene(path, 300)
    assert 450 <= count <= 600


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_ray_counts(gpu, monkeypatch, count):
    """T2: ray counts around a wave and a block, on scene Q."""
    default_env(monkeypatch)
    path = rc.q_path()
    rays, ids, t, bary, occ = (a[:count] for a in rc.host_answers(path, 2500))
    rig = Rig(path)
    got = rig.closest(rays)
    got_occ = rig.occluded(rays)
    rig.close()
    rc.assert_same(got, (ids, t, bary))
    assert np.array_equal(got_occ, occ)


def test_the_answer_does_not_depend_on_the_file_order(gpu, monkeypatch, tmp_path):
    """T3: scene Q written in three orders (identity, reversed, a random permutation): the same
    answers once the ids are mapped back."""
    default_env(monkeypatch)
    v = rc.vertices_of(rc.q_path())
    n = len(v)
    rays, ids, t, bary, occ = rc.host_answers(rc.q_path(), 2500)
    rc.assert_mix(ids, qc.LARGE_IDS)
    orders = {"identity": np.arange(n), "reversed": np.arange(n)[::-1],
              "permuted": np.random.default_rng(4).permutation(n)}
    for name, order in orders.items():
        rig = Rig(write_custom_scene(tmp_path / f"{name}.srt", v[order]))
        got = rig.closest(rays)
        got_occ = rig.occluded(rays)
        rig.close()
        back = np.where(got[0] >= 0, order[np.maximum(got[0], 0)], -1).astype(np.int32)
        rc.assert_same((back, got[1], got[2]), (ids, t, bary))
        assert np.array_equal(got_occ, occ), name


def test_motion(gpu, monkeypatch, tmp_path, capfd):
    """T5: set_vertices (with and without reorder) marks the tree stale; the next query answers as the
    host does on the new vertices; set_camera changes nothing; only the first build allocates."""
    import torch

    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    path = rc.q_path()
    v0 = rc.vertices_of(path)
    rays, ids0, t0, bary0, occ0 = rc.host_answers(path, 2500)
    rc.assert_mix(ids0, qc.LARGE_IDS)
    rig = Rig(path)
    rig.scene.build_rays(rig.stream)
    assert rig.stats(capfd) == (1, 1)
    rc.assert_same(rig.closest(rays), (ids0, t0, bary0))
    cam = list(rig.scene.camera)
    cam[0] += 0.5
    rig.scene.set_camera(cam, stream=rig.stream)
    rc.assert_same(rig.closest(rays), (ids0, t0, bary0))
    assert rig.stats(capfd) == (1, 1)
    rng = np.random.default_rng(9)
    for step, reorder in enumerate((True, False)):
        v = (v0 + rng.uniform(-0.2, 0.2, v0.shape)).astype(f32)
        moved = write_custom_scene(tmp_path / f"moved{step}.srt", v)
        dv = torch.from_numpy(v).cuda()
        rig.scene.set_vertices(dv, reorder=reorder, stream=rig.stream)
        _, ids, t, bary, occ = rc.host_answers(moved, 2500)
        rays_m = rc.mixed_rays(moved, 2500)
        rc.assert_mix(ids, qc.LARGE_IDS)
        rc.assert_same(rig.closest(rays_m), (ids, t, bary))
        assert np.array_equal(rig.occluded(rays_m), occ)
        assert rig.stats(capfd) == (2 + step, 1)
        fresh = Rig(moved)
        rc.assert_same(fresh.closest(rays_m), (ids, t, bary))
        fresh.close()
    rig.close()


def test_edge_cases(gpu, monkeypatch):
    """T6: null handle and pointers, the wrapper's ValueErrors, a scene never prepared, count == 0,
    bary=None, two streams."""
    import torch

    from simpleraytracer_amd import _native

    default_env(monkeypatch)
    L = _native.lib()
    path = rc.q_path()
    rays, ids, t, bary, occ = (a[:300] for a in rc.host_answers(path, 2500))
    rig = Rig(path)  # never prepared
    h = rig.scene.handle
    dr = torch.from_numpy(np.array(rays)).cuda()
    di = torch.empty(300, dtype=torch.int32, device="cuda")
    dt = torch.empty(300, dtype=torch.float32, device="cuda")
    do = torch.empty(300, dtype=torch.uint8, device="cuda")
    for call, msg in (
            (lambda: L.rtrClosestAsync(None, dr.data_ptr(), 300, di.data_ptr(), dt.data_ptr(), None, None), "Bad scene handle"),
            (lambda: L.rtrOccludedAsync(None, dr.data_ptr(), 300, do.data_ptr(), None), "Bad scene handle"),
            (lambda: L.rtrBuildAsync(None, None), "Bad scene handle"),
            (lambda: L.rtrClosestAsync(h, None, 300, di.data_ptr(), dt.data_ptr(), None, None),
             "Bad buffer argument: d_rays is NULL"),
            (lambda: L.rtrClosestAsync(h, dr.data_ptr(), 300, None, dt.data_ptr(), None, None),
             "Bad buffer argument: d_ids is NULL"),
            (lambda: L.rtrClosestAsync(h, dr.data_ptr(), 300, di.data_ptr(), None, None, None),
             "Bad buffer argument: d_t is NULL"),
            (lambda: L.rtrOccludedAsync(h, None, 300, do.data_ptr(), None), "Bad buffer argument: d_rays is NULL"),
            (lambda: L.rtrOccludedAsync(h, dr.data_ptr(), 300, None, None), "Bad buffer argument: d_out is NULL"),
            (lambda: L.rtrClosestAsync(h, dr.data_ptr() + 4, 299, di.data_ptr(), dt.data_ptr(), None, None),
             "Bad buffer argument: d_rays is not 16-byte aligned")):
        assert call() == -1
        assert _native.last_error() == msg
    assert L.rtrClosestAsync(h, None, 0, None, None, None, None) == 0  # count == 0: nothing is read or enqueued
    assert L.rtrOccludedAsync(h, None, 0, None, None) == 0
    s = rig.scene
    with pytest.raises(ValueError, match=r"rays must be \('count', 8\)"):
        s.closest(dr.reshape(-1, 4), di, dt)
    with pytest.raises(ValueError, match="ids must be"):
        s.closest(dr, di[:299], dt)
    with pytest.raises(ValueError, match="t must be torch.float32"):
        s.closest(dr, di, dt.double())
    with pytest.raises(ValueError, match="bary must be"):
        s.closest(dr, di, dt, torch.empty(300, 3, device="cuda"))
    with pytest.raises(ValueError, match="rays must be contiguous"):
        s.closest(torch.empty(8, 300, device="cuda").t(), di, dt)
    with pytest.raises(ValueError, match="must live on cuda:0"):
        s.closest(dr.cpu(), di, dt)
    with pytest.raises(ValueError, match="out must be torch.uint8"):
        s.occluded(dr, di)
    with pytest.raises(ValueError, match="raw pointers carry no count"):
        s.closest(dr.data_ptr(), di.data_ptr(), dt.data_ptr())
    empty = rig.closest(rays[:0])
    assert empty[0].shape == (0,) and rig.occluded(rays[:0]).shape == (0,)
    got = rig.closest(rays, bary=False)
    qc.assert_same(got[0], got[1], ids, t)
    rc.assert_same(rig.closest(rays), (ids, t, bary))
    # two streams: each call is ordered after the scene's previous one, whatever its stream
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        rc.assert_same(rig.closest(rays, stream=s1), (ids, t, bary))
        assert np.array_equal(rig.occluded(rays, stream=s2), occ)
    rig.close()
