#!/usr/bin/env python3
"""G-buffer pass against the deferred shading pass of the same ids (needs an MI355X).

    python tools/gbuffer_probe.py [--launches 20] [--repeats 5] [--triangles 100000] [--out DIR]
                                  [--lib NAME=PATH ...] [--step-timeout 240]

C3 (soup-100k, 1920 x 1080, offsets 0.5), one scene, one stream. Every library measured (the
product build, or each --lib: measurement builds of `make exp`, e.g. EXP_FLAGS=-DSRT_GBUFFER_PIXELS=4)
is one step: a child process of its own under `timeout`, and the first step that fails ends the run.
A step traces the frame's ids once, checks the G-buffer against the traced RGBA frame (albedo.rgb *
normal.w, albedo.a: bit-equal) and its depth against rtqQueryAsync's t, then alternates four cases
within every repeat, each timed with device events around --launches launches after a warm-up:

    shade            srtShadeAsync of the ids: the yardstick, the same gather, 28 B per pixel
                     (8 offset + 4 id in, 16 out)
    gbuffer_all      rtgFrameAsync, all four planes: 56 B per pixel (12 in, 44 out)
    gbuffer_depth    depth only: 16 B per pixel (12 in, 4 out)
    gbuffer_shading  normal + albedo: 44 B per pixel (12 in, 32 out)

Reports, per case, us per launch (median over the repeats), the spread (min, max) and the
compulsory bytes per second (the bytes above; the gathered records are not counted: they are
shared between neighbouring pixels). The sanity condition, stated, not a gate: gbuffer_all's
bytes per second within the repeats' spread of shade's -- below it the pass is latency- or
gather-bound rather than store-bound.
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

BYTES = {"shade": 28, "gbuffer_all": 56, "gbuffer_depth": 16, "gbuffer_shading": 44}


def step(a):
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.device import pixel_positions

    W, H = a.width, a.height
    pixels = W * H
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    scene = srt.DeviceScene(path, 0)
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    f32 = dict(dtype=torch.float32, device=dev)
    off = torch.full((H, W, 2), 0.5, **f32)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    rgba = torch.empty((H, W, 4), **f32)
    shaded = torch.empty((H, W, 4), **f32)
    depth, bary = torch.empty((H, W), **f32), torch.empty((H, W, 2), **f32)
    normal, albedo = torch.empty((H, W, 4), **f32), torch.empty((H, W, 4), **f32)
    scene.trace_ids(off, ids, stream=stream)
    scene.trace(off, rgba, stream=stream)
    cases = {
        "shade": lambda: scene.shade(off, ids, shaded, stream=stream),
        "gbuffer_all": lambda: scene.gbuffer(off, ids, depth, bary, normal, albedo, stream=stream),
        "gbuffer_depth": lambda: scene.gbuffer(off, ids, depth=depth, stream=stream),
        "gbuffer_shading": lambda: scene.gbuffer(off, ids, normal=normal, albedo=albedo, stream=stream),
    }
    # Warm-up launch of each shape, and the answers checked while at it.
    for run in cases.values():
        run()
    pos = torch.from_numpy(pixel_positions(W, H, 0.5)).to(dev)
    q_ids = torch.empty((pixels,), dtype=torch.int32, device=dev)
    q_t = torch.empty((pixels,), **f32)
    scene.query(pos, q_ids, q_t, stream=stream)
    torch.cuda.synchronize()
    composed = torch.cat([albedo[..., :3] * normal[..., 3:], albedo[..., 3:]], dim=-1)
    if not (torch.equal(composed.view(torch.int32), rgba.view(torch.int32)) and torch.equal(shaded, rgba)):
        raise SystemExit("albedo.rgb * normal.w, albedo.a differs from the traced frame")
    if not torch.equal(depth.reshape(-1).view(torch.int32), q_t.view(torch.int32)):
        raise SystemExit("depth differs from the point queries' t")
    hits = int((ids >= 0).sum().item())

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
    out = {"library": a.child, "workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5", "pixels": pixels, "hits": hits,
           "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, v in us.items():
        med = statistics.median(v)
        out["cases"][name] = {"us_per_launch": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                              "bytes_per_pixel": BYTES[name],
                              "gb_per_s": round(BYTES[name] * pixels / med / 1e3, 1),
                              "gb_per_s_min": round(BYTES[name] * pixels / max(v) / 1e3, 1),
                              "gb_per_s_max": round(BYTES[name] * pixels / min(v) / 1e3, 1)}
    c = out["cases"]
    out["all_planes_within_spread_of_shade"] = c["gbuffer_all"]["gb_per_s_max"] >= c["shade"]["gb_per_s_min"]
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"probe_{a.child}.json"), "w") as f:
            json.dump(out, f, indent=1)
    scene.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None, help="directory for one probe_NAME.json per library")
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="a library to measure (SRT_LIB)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        step(a)
        return
    libs = [s.split("=", 1) for s in a.lib] or [["product", ""]]
    for name, lib in libs:
        env = dict(os.environ)
        if lib:
            env["SRT_LIB"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", name,
               "--launches", str(a.launches), "--repeats", str(a.repeats), "--triangles", str(a.triangles),
               "--width", str(a.width), "--height", str(a.height)] + (["--out", a.out] if a.out else [])
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:  # nothing more is started after a step that failed, faulted or timed out
            raise SystemExit(f"step {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
