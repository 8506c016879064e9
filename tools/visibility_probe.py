#!/usr/bin/env python3
"""Sampled visibility: the fused call against the composition it replaces (run on the GPU box).

    python tools/visibility_probe.py [--launches 5] [--repeats 3] [--samples 8 16] [--tmax 0.5] [--out FILE]

C3 (soup-100k, 1920 x 1080, offsets 0.5) in one process, one scene, one stream; the elements are the
frame's pixels with the cull trace's hit ids. For every S of --samples and a cosine hemisphere with
and without a rotation table, three paths to the same `visible` plane:

    fused         scene.visibility_frame                                   (one launch)
    sample_major  scene.generate_rays_frame + scene.occluded + a torch count over the S planes
    pixel_major   the same with the occlusion call reading a pixel-major copy of the rays (the S rays
                  of a pixel side by side: the layout a host-built batch has); the copy is made
                  once, outside the timing

Before anything is timed the three must agree on the bytes. Every case is timed with device events
around --launches launches after a warm-up launch of every shape, the cases alternated within every
repeat. Reports us per launch (median over the repeats, with min and max) and Mrays/s (pixels x S
per launch), the share of occluded rays and the mean of `visible`.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--tmax", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the summary JSON here")
    a = ap.parse_args()
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd import samples as sm

    W, H = a.width, a.height
    pixels = W * H
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    scene = srt.DeviceScene(path, 0)
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    off = torch.full((H, W, 2), 0.5, dtype=torch.float32, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    scene.trace_ids(off, ids, 0, H, variant="cull", stream=stream)
    scene.build_rays(stream)
    torch.cuda.synchronize()
    surface_share = float((ids >= 0).float().mean().item())

    cases, facts = {}, {}
    keep = []
    for S in a.samples:
        table = torch.from_numpy(sm.cosine_hemisphere(S, 1)).to(dev)
        turns = torch.from_numpy(sm.rotations(2)).to(dev)
        rays = torch.empty((S, H, W, 8), dtype=torch.float32, device=dev)
        occ = torch.empty((S * pixels,), dtype=torch.uint8, device=dev)
        fused = torch.empty((H, W), dtype=torch.uint8, device=dev)
        keep += [table, turns, rays, occ, fused]
        for rotated in (False, True):
            gen = srt.Hemisphere(table, 2.0 ** -10, a.tmax, turns if rotated else None)
            tag = f"S{S}_{'rotated' if rotated else 'plain'}"

            def run_fused(gen=gen, fused=fused):
                scene.visibility_frame(off, ids, gen, visible=fused, stream=stream)

            def run_sample_major(gen=gen, rays=rays, occ=occ, S=S):
                scene.generate_rays_frame(off, ids, gen, rays, stream=stream)
                scene.occluded(rays.view(-1, 8), occ, stream=stream)
                return (occ.view(S, pixels) == 0).sum(dim=0, dtype=torch.uint8)

            run_fused()
            want = run_sample_major()
            torch.cuda.synchronize()
            if not torch.equal(fused.view(-1), want):
                raise SystemExit(f"{tag}: the fused call differs from the sample-major composition")
            by_pixel = rays.view(S, pixels, 8).permute(1, 0, 2).contiguous()  # (pixels, S, 8)
            keep.append(by_pixel)

            def run_pixel_major(gen=gen, rays=rays, occ=occ, S=S, by_pixel=by_pixel):
                scene.generate_rays_frame(off, ids, gen, rays, stream=stream)
                scene.occluded(by_pixel.view(-1, 8), occ, stream=stream)
                return (occ.view(pixels, S) == 0).sum(dim=1, dtype=torch.uint8)

            got = run_pixel_major()
            torch.cuda.synchronize()
            if not torch.equal(got, want):
                raise SystemExit(f"{tag}: the pixel-major composition differs from the sample-major one")
            mean_visible = float(want.float().mean().item())
            facts[tag] = {"occluded_share": round(1.0 - mean_visible / S, 4), "mean_visible": round(mean_visible, 3)}
            cases[f"{tag}_fused"] = (S, run_fused)
            cases[f"{tag}_sample_major"] = (S, run_sample_major)
            cases[f"{tag}_pixel_major"] = (S, run_pixel_major)

    us = {name: [] for name in cases}
    for _ in range(a.repeats):
        for name, (_, call) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _k in range(a.launches):
                call()
            e1.record(stream)
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    out = {"workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5, cosine hemisphere, range [2^-10, {a.tmax}]",
           "library": os.path.basename(os.path.dirname(os.environ["SRT_LIB"])) if os.environ.get("SRT_LIB") else "product build", "pixels": pixels,
           "surface_share": round(surface_share, 4), "launches": a.launches, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "facts": facts, "cases": {}, "fused_over_best_composition": {}}
    for name, v_us in us.items():
        med = statistics.median(v_us)
        rays_per_launch = cases[name][0] * pixels
        out["cases"][name] = {"us_per_launch": round(med, 1), "us_min": round(min(v_us), 1), "us_max": round(max(v_us), 1),
                              "mrays_per_s": round(rays_per_launch / med, 1)}
        print(json.dumps({name: out["cases"][name]}), flush=True)
    for tag in facts:
        best = min(out["cases"][f"{tag}_sample_major"]["us_per_launch"], out["cases"][f"{tag}_pixel_major"]["us_per_launch"])
        out["fused_over_best_composition"][tag] = round(out["cases"][f"{tag}_fused"]["us_per_launch"] / best, 3)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    scene.close()


if __name__ == "__main__":
    main()
