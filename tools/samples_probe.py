#!/usr/bin/env python3
"""Multi-sample frames against the detours they replace (needs an MI355X).

    python tools/samples_probe.py [--samples 1,2,4,8,16] [--launches 20] [--repeats 5] [--triangles 100000]
                                  [--out DIR] [--lib NAME=PATH ...] [--step-timeout 420]

C3 (soup-100k, 1920 x 1080), stratified sample offsets (samples.stratified_offsets), one scene, one
stream. Every library measured (the product build, or each --lib: measurement builds of `make exp`,
e.g. EXP_FLAGS=-DSRT_RESOLVE_GROUP=8) is one step: a child process of its own under `timeout`, and
the first step that fails ends the run. For every S a step traces the S id planes and the S RGBA
frames once, checks the resolve (bit-equal to rtsRenderAsync's; within (S + 1) 2^-24 of the float64
mean of the traced frames; for S = 1 bit-equal rgb to srtShadeAsync), then alternates four cases within
every repeat, each timed with device events around --launches launches after a warm-up:

    shade      S launches of srtShadeAsync on the same ids and offsets, an RGBA frame each: the
               yardstick of the resolve, the same gathers, 28 S bytes per pixel
    resolve    rtsResolveAsync: 12 S + 16 bytes per pixel (8 offset + 4 id in per sample, 16 out)
    detour     S launches of srtTraceAsync into RGBA frames, then torch.mean over them: what a caller
               without this family runs for an S-sample frame
    render     rtsRenderAsync: the S id planes traced in batches, then resolved

Reports, per case, us per launch (median over the repeats), the spread (min, max) and, for shade and
resolve, the compulsory bytes per second (the bytes above; the gathered shading-table rows are not
counted). The sanity condition, stated, not a gate: resolve takes less time than the S shade
launches it replaces -- the same gathers and, from S = 8 on, half the bytes; if it does not, it is
latency-bound.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def step(a):
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.samples import stratified_offsets

    W, H = a.width, a.height
    pixels = W * H
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    scene = srt.DeviceScene(path, 0)
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"library": a.child, "workload": f"soup-{a.triangles} {W}x{H}, stratified offsets", "pixels": pixels,
           "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "samples": {}}
    for S in a.sample_counts:
        off = [torch.from_numpy(o).to(dev) for o in stratified_offsets(W, H, S, seed=S)]
        ids = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(S)]
        ids_r = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(S)]
        frames = torch.empty((S, H, W, 4), **f32)
        shaded = torch.empty((S, H, W, 4), **f32)
        resolved, rendered, mean = (torch.empty((H, W, 4), **f32) for _ in range(3))

        def shade():
            for s in range(S):
                scene.shade(off[s], ids[s], shaded[s], stream=stream)

        def detour():
            for s in range(S):
                scene.trace(off[s], frames[s], stream=stream)
            torch.mean(frames, dim=0, out=mean)

        cases = {
            "shade": shade,
            "resolve": lambda: scene.resolve(off, ids, resolved, stream=stream),
            "detour": detour,
            "render": lambda: scene.render_samples(off, ids_r, rendered, stream=stream),
        }
        # The id planes, then a warm-up launch of each case, and the answers checked while at it.
        for s in range(S):
            scene.trace_ids(off[s], ids[s], stream=stream)
        for run in cases.values():
            run()
        torch.cuda.synchronize()
        if not all(torch.equal(ids[s], ids_r[s]) for s in range(S)):
            raise SystemExit(f"S={S}: rtsRenderAsync's id planes differ from srtTraceIdsAsync's")
        if not torch.equal(rendered.view(torch.int32), resolved.view(torch.int32)):
            raise SystemExit(f"S={S}: rtsRenderAsync differs from trace_ids + rtsResolveAsync")
        if not torch.equal(shaded.view(torch.int32), frames.view(torch.int32)):
            raise SystemExit(f"S={S}: srtShadeAsync differs from the traced frames")
        want = frames[..., :3].to(torch.float64).mean(dim=0)
        err = float((resolved[..., :3].to(torch.float64) - want).abs().max().item())
        if err > (S + 1) * 2.0 ** -24:  # S - 1 adds of sums <= S and one division, each within half an ulp
            raise SystemExit(f"S={S}: the resolve is {err:.3e} from the float64 mean of the traced frames")
        cover = (frames[..., 3] >= 0).sum(dim=0).to(torch.float32) / S
        if not torch.equal(resolved[..., 3], cover):
            raise SystemExit(f"S={S}: alpha is not the coverage")
        if S == 1 and not torch.equal(resolved[..., :3].view(torch.int32), shaded[0, ..., :3].view(torch.int32)):
            raise SystemExit("S=1: rgb differs from srtShadeAsync's")

        us = {name: [] for name in cases}
        for _ in range(a.repeats):
            for name, run in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _k in range(a.launches):
                    run()
                e1.record(stream)
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        row = {"max_err_vs_float64_mean": err, "partial_coverage": float(((cover > 0) & (cover < 1)).float().mean().item()),
               "cases": {}}
        bytes_pp = {"shade": 28 * S, "resolve": 12 * S + 16}
        for name, v in us.items():
            med = statistics.median(v)
            c = {"us_per_launch": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
            if name in bytes_pp:
                c["bytes_per_pixel"] = bytes_pp[name]
                c["gb_per_s"] = round(bytes_pp[name] * pixels / med / 1e3, 1)
            row["cases"][name] = c
        c = row["cases"]
        row["resolve_faster_than_shade_launches"] = c["resolve"]["us_max"] < c["shade"]["us_min"]
        row["render_faster_than_detour"] = c["render"]["us_max"] < c["detour"]["us_min"]
        out["samples"][str(S)] = row
        del off, ids, ids_r, frames, shaded, resolved, rendered, mean
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"probe_{a.child}.json"), "w") as f:
            json.dump(out, f, indent=1)
    scene.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="1,2,4,8,16", help="comma-separated sample counts")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None, help="directory for one probe_NAME.json per library")
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="a library to measure (SRT_LIB)")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds per library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.sample_counts = [int(s) for s in a.samples.split(",")]
    if a.child is not None:
        step(a)
        return
    libs = [s.split("=", 1) for s in a.lib] or [["product", ""]]
    for name, lib in libs:
        env = dict(os.environ)
        if lib:
            env["SRT_LIB"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", name,
               "--samples", a.samples, "--launches", str(a.launches), "--repeats", str(a.repeats),
               "--triangles", str(a.triangles), "--width", str(a.width), "--height", str(a.height)]
        cmd += ["--out", a.out] if a.out else []
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:  # nothing more is started after a step that failed, faulted or timed out
            raise SystemExit(f"step {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
