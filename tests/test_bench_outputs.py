"""bench.py's plain run, --dump-outputs and --full.

A plain run times the steps and prints the headline line only; --dump-outputs writes frames of the last
timed step (checked here against the oracle); --full adds the verification, the roofline and stage
passes, the legs and the CPU baseline. Small frames: 320 x 200, 2 000 triangles, 8 frames per step."""
from __future__ import annotations

import json
import os
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--width", "320", "--height", "200", "--triangles", "2000",
         "--frames-per-step", "8"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY = {"roofline", "roofline_single_frame", "stages_ms", "brute_force_equivalent", "verified", "verify",
             "single_queue", "cpu_baseline", "e2e_ml_api"}


def run_bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), *args], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


class StubEngine:
    """read_frame of frame k: every channel of every pixel holds k."""

    def __init__(self, height, width, batch):
        self.height, self.width, self.batch, self.options = height, width, batch, {"split": "bands"}

    def read_frame(self, k):
        return np.full((self.height, self.width, 4), float(k), np.float32)


@pytest.mark.parametrize("height,width,batch", [(1080, 1920, 256), (2160, 3840, 64), (32, 64, 1)])
def test_dump_outputs_is_seeded_and_bounded(tmp_path, height, width, batch):
    """The dump reads frames of the last timed step only, picks the same frames and rows on every call,
    writes float32 arrays and stays under 64 MB at the headline size, at 4K (rows of the first
    frame sampled) and for a one-frame step (no further frames)."""
    sys.path.insert(0, str(REPO))
    import bench

    job = types.SimpleNamespace(world=1, ranked=False, rank=0)
    a = types.SimpleNamespace(warmup=2, steps=3)
    outs = [bench.dump_outputs(job, StubEngine(height, width, batch), a, tmp_path / d) for d in ("a", "b")]
    assert {**outs[0], "dir": None} == {**outs[1], "dir": None}
    first = (a.warmup + a.steps - 1) * batch
    assert outs[0]["frames"][0] == 0 and all(0 <= k < batch for k in outs[0]["frames"])
    assert len(set(outs[0]["frames"])) == len(outs[0]["frames"]) == min(16, batch)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(outs[0]["files"]) == (["frame.npy", "sample.npy"] if batch > 1 else ["frame.npy"])
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64_000_000
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y)
    frame = np.load(tmp_path / "a" / "frame.npy")
    assert np.all(frame == first) and frame.shape == (min(height, 48_000_000 // (width * 16)), width, 4)
    if batch > 1:
        sample = np.load(tmp_path / "a" / "sample.npy")
        assert sample.shape == (len(outs[0]["frames"]) - 1, 16, width, 4)
        assert [int(i) for i in sample[:, 0, 0, 0]] == [first + k for k in outs[0]["frames"][1:]]
        assert np.all(sample == sample[:, :1, :1, :1])


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return run_bench(*SMALL, "--dump-outputs", str(d)), d


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(gpu, plain_run):
    line, _ = plain_run
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line), sorted(line)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step state the same timed steps: 8 frames of 320 x 200 rays per step
    assert line["value"] == pytest.approx(8 * 320 * 200 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)


@pytest.mark.gpu
def test_dumped_frames_match_the_oracle(gpu, plain_run, tmp_path):
    """Every frame of a step renders the same view of the same soup with uniform 0.5 offsets: the dumped
    first frame and the sampled rows of the others against the oracle's render of that scene."""
    import simpleraytracer_amd as srt
    from oracle.srt_oracle import OracleScene

    line, d = plain_run
    assert sorted(p.name for p in d.iterdir()) == sorted(line["outputs"]["files"])
    ref = OracleScene(srt.write_scene(str(tmp_path / "soup.srt"), "soup", 2000)).render(320, 200)
    frame, sample = np.load(d / "frame.npy"), np.load(d / "sample.npy")
    assert frame.dtype == sample.dtype == np.float32 and frame.shape == (200, 320, 4) and sample.shape == (7, 16, 320, 4)
    assert np.array_equal(frame[..., 3], ref[..., 3]) and len(np.unique(frame[..., 3])) > 100
    assert float(np.abs(frame[..., :3] - ref[..., :3]).max()) <= 1e-5
    sys.path.insert(0, str(REPO))
    import bench

    frame_rows, others, sample_rows = bench.dump_plan(200, 320, 8)
    assert list(frame_rows) == list(range(200)) and [0, *others] == line["outputs"]["frames"]
    assert len(sample_rows) == 7 and len({tuple(r) for r in sample_rows}) > 1
    for got, rows in zip(sample, sample_rows):  # 16 seeded rows of each frame
        assert len(set(rows)) == 16 and list(rows) == sorted(rows)
        assert np.array_equal(got[..., 3], ref[rows, :, 3])
        assert float(np.abs(got[..., :3] - ref[rows, :, :3]).max()) <= 1e-5


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_legs(gpu):
    """--full with its slowest parts switched off by their own options (the ml* API rates, the other trace
    variants, and the CPU baseline, which test_bench_errors.py times on its own): every other moved
    field is back."""
    line = run_bench(*SMALL, "--full", "--brute-steps", "0", "--no-e2e", "--no-cpu-baseline")
    assert HEADLINE | FULL_ONLY - {"e2e_ml_api", "cpu_baseline"} <= set(line), sorted(FULL_ONLY - set(line))
    assert line["full"] is True and line["verified"] is True and line["verify"]["mismatches"] == 0
    assert line["value"] > 0 and line["roofline"]["kernel_ms"] > 0 and line["stages_ms"]["trace_kernel"] > 0
    assert line["single_queue"]["mrays_per_s"] > 0 and line["c2_cornell"]["mrays_per_s"] > 0
