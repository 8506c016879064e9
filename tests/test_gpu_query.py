"""Point queries on the device (include/srt_query.h rtqQueryAsync; query.hip QueryKernel): the
closest hit at arbitrary image positions of the prepared frame, answered from the shared setup's
per-tile lists.

Every comparison is exact -- ids equal, t equal on the uint32 view -- against the CPU oracle's
closest_hit over the oracle's own edge records; nothing is excluded. `how` (0 = answered from the
tile's list, 1 = every record streamed) keeps the tests from passing on a kernel that streams
everything, the setup counters (SRT_SETUP_LOG=1) from passing on a build per call.

Frames are 200 x 150 -- 4 x 10 tiles of 64 x 16, the last column and row partial -- unless a test
says otherwise; scene Q and the position families are tests/query_cases.py's.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import query_cases as qc

pytestmark = pytest.mark.gpu

W, H = qc.W, qc.H
W2, H2 = 333, 170


@pytest.fixture(scope="module")
def scene_q(tmp_path_factory):
    return qc.write_scene_q(tmp_path_factory.mktemp("query") / "q.srt")


class Rig:
    """One scene on cuda:0 and its stream; query() and trace_ids() return numpy arrays."""

    def __init__(self, path, w=None, h=None):
        import torch

        import simpleraytracer_amd as srt

        self.torch = torch
        self.scene = srt.DeviceScene(path, 0)
        self.stream = torch.cuda.current_stream()
        if w is not None:
            self.prepare(w, h)

    def prepare(self, w, h):
        self.w, self.h = w, h
        self.scene.prepare(w, h, self.stream)

    def query(self, pos, stream=None):
        torch = self.torch
        n = len(pos)
        p = torch.from_numpy(np.array(pos, np.float32)).cuda()  # (a copy: the shared cases are read-only)
        ids = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        t = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        how = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.scene.query(p, ids, t, how, stream=self.stream if stream is None else stream)
        torch.cuda.synchronize()
        return ids.cpu().numpy(), t.cpu().numpy(), how.cpu().numpy()

    def trace_ids(self, offsets, variant="cull", r0=0, rows=None):
        torch = self.torch
        rows = self.h - r0 if rows is None else rows
        off = torch.from_numpy(np.ascontiguousarray(offsets[r0:r0 + rows])).cuda()
        out = torch.full((rows, self.w), -7, dtype=torch.int32, device="cuda")
        self.scene.trace_ids(off, out, r0, rows, variant=variant, stream=self.stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def stats(self, capfd):
        lines = re.findall(r"srt setup: scene \S+ builds (\d+) shared_frames (\d+) per_frame_frames (\d+)",
                           capfd.readouterr().err)
        assert lines, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
        return tuple(int(v) for v in lines[-1])

    def close(self):
        self.scene.close()


def default_env(monkeypatch):
    for name in ("SRT_SETUP", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_TRACE_RECORDS"):
        monkeypatch.delenv(name, raising=False)


def test_pixel_grid_equals_the_trace_and_the_oracle(gpu, scene_q, monkeypatch, capfd):
    """Every pixel position of a frame with random offsets: the ids the cull trace stores, (id, t)
    the oracle's, all answered from the lists, and the query and the trace share one build."""
    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    pos, want_ids, want_t = qc.cached_answers(scene_q, W, H, "pixels")
    qc.assert_mix(want_ids)
    rig = Rig(scene_q, W, H)
    ids, t, how = rig.query(pos)
    traced = rig.trace_ids(qc.random_offsets(W, H, 3))
    builds = rig.stats(capfd)[0]
    rig.close()
    assert len(pos) == W * H == 30000
    assert np.array_equal(ids.reshape(H, W), traced)
    qc.assert_same(ids, t, want_ids, want_t)
    assert np.all(how == 0)
    assert builds == 1


def test_arbitrary_and_boundary_positions(gpu, scene_q, monkeypatch):
    """Random positions, exactly 0 and 1, every tile boundary with its float neighbours, and the
    out-of-range values: the oracle's answers; from the lists exactly for positions in [0, 1]^2."""
    default_env(monkeypatch)
    pos, want_ids, want_t = qc.cached_answers(scene_q, W, H, "mixed")
    qc.assert_mix(want_ids)
    rig = Rig(scene_q, W, H)
    ids, t, how = rig.query(pos)
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    inside = qc.in_range(pos)
    assert inside.sum() >= 2000 and (~inside).sum() >= len(qc.OUT_OF_RANGE) ** 2
    assert np.array_equal(how, np.where(inside, 0, 1).astype(np.uint8))


def test_overflowed_lists_stream(gpu, scene_q, monkeypatch):
    """Lists capped at 8 entries: a query in an overflowed tile streams, one in a short tile does not."""
    default_env(monkeypatch)
    monkeypatch.setenv("SRT_CULL_BIN_CAP", "8")
    pos, want_ids, want_t = qc.cached_answers(scene_q, W, H, "mixed")
    qc.assert_mix(want_ids)
    rig = Rig(scene_q, W, H)
    ids, t, how = rig.query(pos)
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    inside = qc.in_range(pos)
    assert (how[inside] == 1).any() and (how[inside] == 0).any()
    assert np.all(how[~inside] == 1)


@pytest.mark.parametrize("records", ["stored", "recompute"])
def test_record_sources(gpu, scene_q, monkeypatch, records):
    default_env(monkeypatch)
    monkeypatch.setenv("SRT_TRACE_RECORDS", records)
    pos, want_ids, want_t = qc.cached_answers(scene_q, W, H, "mixed")
    qc.assert_mix(want_ids)
    rig = Rig(scene_q, W, H)
    ids, t, how = rig.query(pos)
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    assert np.array_equal(how == 0, qc.in_range(pos))


@pytest.mark.parametrize("name,value", [("SRT_SETUP", "frame"), ("SRT_CULL_BIN", "0")])
def test_no_usable_setup_streams_every_query(gpu, scene_q, monkeypatch, name, value):
    default_env(monkeypatch)
    monkeypatch.setenv(name, value)
    pos, want_ids, want_t = qc.cached_answers(scene_q, W, H, "mixed")
    pos, want_ids, want_t = pos[:2000], want_ids[:2000], want_t[:2000]  # the random in-range positions
    qc.assert_mix(want_ids)
    assert qc.in_range(pos).all()
    rig = Rig(scene_q, W, H)
    ids, t, how = rig.query(pos)
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    assert np.all(how == 1)


def test_reprepare_and_mixing_with_traces(gpu, scene_q, monkeypatch, capfd):
    """query -> whole-frame trace -> band trace -> prepare(333, 170) -> query on another stream: each
    correct, two builds of the setup in all (one per prepared frame)."""
    import torch

    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    pos, want_ids, want_t = qc.cached_answers(scene_q, W, H, "mixed")
    off = qc.random_offsets(W, H, 3)
    _, pixel_ids, _ = qc.cached_answers(scene_q, W, H, "pixels")
    pos2 = qc.mixed_positions(W2, H2, seed=9)
    want2_ids, want2_t = qc.oracle_answers(scene_q, W2, H2, pos2)
    qc.assert_mix(want_ids)
    qc.assert_mix(want2_ids)
    rig = Rig(scene_q, W, H)
    ids, t, how = rig.query(pos)
    frame = rig.trace_ids(off)
    band = rig.trace_ids(off, r0=40, rows=78)  # rows 40..117
    rig.prepare(W2, H2)
    other = torch.cuda.Stream()
    ids2, t2, how2 = rig.query(pos2, stream=other)
    builds = rig.stats(capfd)[0]
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    assert np.array_equal(frame, pixel_ids.reshape(H, W))
    assert np.array_equal(band, pixel_ids.reshape(H, W)[40:118])
    qc.assert_same(ids2, t2, want2_ids, want2_t)
    assert np.array_equal(how2 == 0, qc.in_range(pos2))
    assert builds == 2


def test_long_lists(gpu, scenes, monkeypatch):
    """soup-100k at 1920 x 1080: the centre tiles' lists hold several hundred candidates, so a wave
    walks several rounds. 4 096 random positions and the pixels of rows 536..539, columns 0..1023."""
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    w, h = 1920, 1080
    rng = np.random.default_rng(17)
    pixels = device.pixel_positions(w, h, 0.5).reshape(h, w, 2)[536:540, :1024].reshape(-1, 2)
    pos = np.concatenate([rng.random((4096, 2), dtype=np.float32), pixels])
    assert len(pos) == 8192
    want_ids, want_t = qc.oracle_answers(scenes["soup100k"], w, h, pos)
    assert (want_ids >= 0).sum() >= 0.10 * len(pos) and (want_ids < 0).sum() >= 0.10 * len(pos)
    rig = Rig(scenes["soup100k"], w, h)
    ids, t, how = rig.query(pos)
    rig.close()
    qc.assert_same(ids, t, want_ids, want_t)
    assert np.all(how == 0)


def test_edge_cases(gpu, scene_q, scenes, monkeypatch):
    import ctypes

    import torch

    from simpleraytracer_amd import SrtError, _native

    default_env(monkeypatch)
    L = _native.lib()
    # a scene that was never prepared
    rig = Rig(scene_q)
    p = torch.zeros((4, 2), dtype=torch.float32, device="cuda")
    ids = torch.zeros((4,), dtype=torch.int32, device="cuda")
    t = torch.zeros((4,), dtype=torch.float32, device="cuda")
    how = torch.zeros((4,), dtype=torch.uint8, device="cuda")
    with pytest.raises(SrtError, match=r"Query: Prepare\(\) has not been called"):
        rig.scene.query(p, ids, t, how)
    rig.prepare(W, H)
    # count == 0: a no-op
    e2 = torch.empty((0, 2), dtype=torch.float32, device="cuda")
    rig.scene.query(e2, torch.empty((0,), dtype=torch.int32, device="cuda"),
                    torch.empty((0,), dtype=torch.float32, device="cuda"))
    assert L.rtqQueryAsync(rig.scene.handle, None, 0, None, None, None, None) == 0
    # null arguments
    assert L.rtqQueryAsync(None, p.data_ptr(), 4, ids.data_ptr(), t.data_ptr(), None, None) == -1
    assert _native.last_error() == "Bad scene handle"
    for k, name in enumerate(("d_positions", "d_ids", "d_t")):
        args = [p.data_ptr(), ids.data_ptr(), t.data_ptr()]
        args[k] = None
        assert L.rtqQueryAsync(rig.scene.handle, args[0], 4, args[1], args[2], None, None) == -1
        assert name in _native.last_error()
    # the wrapper's buffer checks
    with pytest.raises(ValueError):
        rig.scene.query(torch.zeros((4, 3), dtype=torch.float32, device="cuda"), ids, t)
    with pytest.raises(ValueError):
        rig.scene.query(p, torch.zeros((5,), dtype=torch.int32, device="cuda"), t)
    with pytest.raises(ValueError):
        rig.scene.query(p, ids.to(torch.int64), t)
    with pytest.raises(ValueError):
        rig.scene.query(p, ids, t, how.to(torch.int32))
    with pytest.raises(ValueError):
        rig.scene.query(p.cpu(), ids, t)
    # how is optional, and the valid call still works after the refused ones
    rig.scene.query(p, ids, t)
    torch.cuda.synchronize()
    want_ids, want_t = qc.oracle_answers(scene_q, W, H, np.zeros((4, 2), np.float32))
    qc.assert_same(ids.cpu().numpy(), t.cpu().numpy(), want_ids, want_t)
    rig.close()
    # the single-triangle scene: every list has one entry or none
    pos = qc.mixed_positions(W, H)
    want_ids, want_t = qc.oracle_answers(scenes["triangle"], W, H, pos)
    assert (want_ids == 0).any() and (want_ids == -1).any()
    rig = Rig(scenes["triangle"], W, H)
    got_ids, got_t, got_how = rig.query(pos)
    rig.close()
    qc.assert_same(got_ids, got_t, want_ids, want_t)
    assert np.array_equal(got_how == 0, qc.in_range(pos))
