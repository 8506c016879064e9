#!/usr/bin/env python3
"""Vertex-attribute pass against the G-buffer pass and against the composition it replaces (needs
an MI355X).

    python tools/surface_probe.py [--launches 20] [--repeats 5] [--triangles 100000] [--texture 1024]
                                  [--out DIR] [--lib NAME=PATH ...] [--step-timeout 240]

C3 (soup-100k, 1920 x 1080, offsets 0.5), one scene, one stream, random corner normals and uvs and
a random --texture x --texture texture (repeat, bilinear). Every library measured (the product
build, or each --lib: measurement builds of `make exp`, e.g. EXP_FLAGS=-DSRT_SURFACE_PIXELS=4) is
one step: a child process of its own under `timeout`, and the first step that fails ends the run. A
step traces the frame's ids once, checks the surface call's fallback (no tables) against the traced
RGBA frame on the bits and the composition against the fused call within 5e-3, then alternates the
cases within every repeat, each timed with device events around --launches launches after a warm-up:

    surface_shading  rtvSurfaceFrameAsync, normal + albedo -- what the composition produces: 44 B
                     per pixel (8 offset + 4 id in, 32 out)
    surface_rgba     rgba only: 28 B per pixel (12 in, 16 out)
    surface_all      normal, albedo, rgba and uv: 68 B per pixel (12 in, 56 out)
    gbuffer_all      rtgFrameAsync, all four planes: the yardstick, 56 B per pixel (12 in, 44 out)
    composition      what the fused call replaces: rtgFrameAsync (bary), then in torch the gathers of
                     the corner rows by id, the interpolation, the normalisation and cosine, and a
                     bilinear repeat lookup -- smooth normal and textured albedo, 44 B per pixel
                     compulsory, every intermediate plane through HBM

Reports, per case, us per launch (median over the repeats), the spread (min, max) and the
compulsory bytes per second (the bytes above; the gathered rows and texels are not counted). The
statement to make or refute, stated, not a gate: surface_shading beats composition.
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

BYTES = {"surface_shading": 44, "surface_rgba": 28, "surface_all": 68, "gbuffer_all": 56, "composition": 44}


def step(a):
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.device import scene_frame

    W, H = a.width, a.height
    pixels = W * H
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    scene = srt.DeviceScene(path, 0)
    n = scene.triangles
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    f32 = dict(dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    normals = torch.rand((n, 3, 3), generator=gen, **f32) * 2 - 1
    uvs = torch.rand((n, 3, 2), generator=gen, **f32) * 4 - 1.5
    T = a.texture
    tex = torch.rand((T, T, 4), generator=gen, **f32)
    surface = srt.Surface(normals, uvs, tex)
    off = torch.full((H, W, 2), 0.5, **f32)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    traced = torch.empty((H, W, 4), **f32)
    depth, bary, uv = torch.empty((H, W), **f32), torch.empty((H, W, 2), **f32), torch.empty((H, W, 2), **f32)
    normal, albedo, rgba = (torch.empty((H, W, 4), **f32) for _ in range(3))
    g_normal, g_albedo = torch.empty((H, W, 4), **f32), torch.empty((H, W, 4), **f32)
    scene.trace_ids(off, ids, stream=stream)
    scene.trace(off, traced, stream=stream)
    origin, base, du, dv = (torch.tensor(v, **f32) for v in scene_frame(path, W, H))
    fx = ((torch.arange(W, **f32) + 0.5) / W)[None, :, None]
    fy = ((torch.arange(H, **f32) + 0.5) / H)[:, None, None]
    d = base + fx * du + fy * dv  # (H, W, 3)
    d = d / d.norm(dim=-1, keepdim=True)
    composed = {}

    def composition():
        scene.gbuffer(off, ids, bary=bary, stream=stream)
        hit = ids >= 0
        row = ids.clamp(min=0).long()
        w1, w2 = bary[..., 0:1], bary[..., 1:2]
        w0 = 1 - w1 - w2
        cn, ct = normals[row], uvs[row]  # the gathers: (H, W, 3, 3), (H, W, 3, 2)
        ns = w0 * cn[..., 0, :] + w1 * cn[..., 1, :] + w2 * cn[..., 2, :]
        st = w0 * ct[..., 0, :] + w1 * ct[..., 1, :] + w2 * ct[..., 2, :]
        unit = ns / ns.norm(dim=-1, keepdim=True)
        nd = (unit * d).sum(-1, keepdim=True)
        unit = torch.where(nd > 0, -unit, unit)
        r = st - st.floor()
        x = r * T - 0.5
        x0 = x.floor()
        fr = x - x0
        i0 = x0.long() % T
        i1 = (i0 + 1) % T
        ax, ay = fr[..., 0:1], fr[..., 1:2]
        top = tex[i0[..., 1], i0[..., 0]] * (1 - ax) + tex[i0[..., 1], i1[..., 0]] * ax
        bot = tex[i1[..., 1], i0[..., 0]] * (1 - ax) + tex[i1[..., 1], i1[..., 0]] * ax
        texel = top * (1 - ay) + bot * ay
        composed["normal"] = torch.where(hit[..., None], torch.cat([unit, nd.abs().clamp(max=1)], -1),
                                         torch.tensor([0.0, 0.0, 0.0, 1.0], **f32))
        composed["albedo"] = torch.where(hit[..., None], torch.cat([texel[..., :3], ids[..., None].float()], -1),
                                         traced)

    cases = {
        "surface_shading": lambda: scene.surface_frame(off, ids, surface, normal=normal, albedo=albedo, stream=stream),
        "surface_rgba": lambda: scene.surface_frame(off, ids, surface, rgba=rgba, stream=stream),
        "surface_all": lambda: scene.surface_frame(off, ids, surface, normal, albedo, rgba, uv, stream=stream),
        "gbuffer_all": lambda: scene.gbuffer(off, ids, depth, bary, g_normal, g_albedo, stream=stream),
        "composition": composition,
    }
    # The answers checked first: the fallback on the bits, the composition within a tolerance.
    scene.surface_frame(off, ids, srt.Surface(), rgba=rgba, stream=stream)
    torch.cuda.synchronize()
    if not torch.equal(rgba.view(torch.int32), traced.view(torch.int32)):
        raise SystemExit("the surface call without tables differs from the traced frame")
    for run in cases.values():  # (a warm-up launch of each shape as well)
        run()
    torch.cuda.synchronize()
    away = normal[..., 3:] > 1e-3  # (where the cosine is not near zero: there the normal's sign is not in doubt)
    err_n = float(((composed["normal"] - normal).abs() * away).max())
    err_a = float((composed["albedo"] - albedo).abs().max())
    if not (err_n <= 5e-3 and err_a <= 5e-3):
        raise SystemExit(f"the composition differs from the fused call: normal {err_n:.3e}, albedo {err_a:.3e}")
    if not torch.equal(torch.cat([albedo[..., :3] * normal[..., 3:], albedo[..., 3:]], -1).view(torch.int32),
                       rgba.view(torch.int32)):
        raise SystemExit("rgba differs from albedo.rgb * normal.w, albedo.a")
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
    out = {"library": a.child, "workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5, texture {T}x{T}",
           "pixels": pixels, "hits": hits, "launches": a.launches, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "composition_error": {"normal": err_n, "albedo": err_a},
           "cases": {}}
    for name, v in us.items():
        med = statistics.median(v)
        out["cases"][name] = {"us_per_launch": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                              "bytes_per_pixel": BYTES[name],
                              "gb_per_s": round(BYTES[name] * pixels / med / 1e3, 1),
                              "gb_per_s_min": round(BYTES[name] * pixels / max(v) / 1e3, 1),
                              "gb_per_s_max": round(BYTES[name] * pixels / min(v) / 1e3, 1)}
    c = out["cases"]
    out["fused_beats_composition"] = c["surface_shading"]["us_max"] < c["composition"]["us_min"]
    out["composition_over_fused"] = round(c["composition"]["us_per_launch"] / c["surface_shading"]["us_per_launch"], 2)
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
    ap.add_argument("--texture", type=int, default=1024, help="texels per side")
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
               "--width", str(a.width), "--height", str(a.height), "--texture", str(a.texture)] + \
              (["--out", a.out] if a.out else [])
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:  # nothing more is started after a step that failed, faulted or timed out
            raise SystemExit(f"step {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
