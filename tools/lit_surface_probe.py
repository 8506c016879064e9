#!/usr/bin/env python3
"""Lit-surface time against the composition it replaces and against direct lighting (needs an MI355X).

    python tools/lit_surface_probe.py [--mix spots|point|full] [--lights 4] [--texture 64,1024]
                                      [--launches 20] [--repeats 5] [--out DIR] [--lib NAME=PATH ...]
                                      [--step-timeout 300]

C3 (soup-100k, 1920 x 1080, offsets 0.5), one process per library, one stream. The lights are
tools/lighting_probe.py's (its mixes, ring of spot lights and point lights inside the soup); the
surface is random corner normals and uvs and, for every T of --texture, a random T x T texture
(64: 64 KB, 1024: 16 MB; repeat, bilinear). Every library measured (the product build, or each
--lib: measurement builds of `make exp`, e.g. EXP_FLAGS=-DSRT_LITSURFACE_GATHER=1) is one step: a
child process of its own under `timeout`, and the first step that fails ends the run.

Cases, alternated within every repeat, each timed with device events around --launches launches
after a warm-up launch of each shape:

    fused            rtpLightSurfaceAsync, normals + uvs + texture, RGBA only
    fused_classes    the same with the L class planes
    fused_specular   the same as `fused` with a material (exponent 2^5)
    bare             rtpLightSurfaceAsync with no surface and no material      -- comparison (b)
    lighting         rtdLightAsync, RGBA only                                   -- comparison (b)
    surface          rtvSurfaceFrameAsync, normal + albedo
    back_to_back     `lighting` then `surface`: the two launches the fused call stands in for
    composition      what the fused call replaces: rtdLightAsync with class planes, rtvSurfaceFrameAsync
                     (normal, albedo), rtgFrameAsync (depth, normal), and in torch P = eye + depth d, then per
                     light q, the facing test, the smooth cosine, the weight and the accumulation, and
                     albedo . E -- every intermediate plane through HBM                -- comparison (a)

Before timing: `bare` must equal `lighting` on the bits and the fused class planes rtdLightAsync's
(the probe refuses to go on otherwise); the fused RGBA is compared with the composition's (the
largest difference is reported: the composition's arithmetic is torch's, not the definition's).
Reports, per case, us per launch (median over the repeats) and the spread (min, max). The
expectation to make or refute, stated, not a gate: `fused` costs less than `back_to_back`.
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
sys.path.insert(0, os.path.join(REPO, "tools"))


def step(a):
    import torch

    import simpleraytracer_amd as srt
    from lighting_probe import AMBIENT, COLORS, POINTS, spot_camera
    from simpleraytracer_amd.device import scene_frame

    W, H = a.width, a.height
    dev = torch.device("cuda", 0)
    f32 = dict(dtype=torch.float32, device=dev)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    stream = torch.cuda.current_stream()
    view = srt.DeviceScene(path, 0)
    view.prepare(W, H, stream)
    n = view.triangles
    off = torch.full((H, W, 2), 0.5, **f32)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    view.trace_ids(off, ids, 0, H, variant="cull", stream=stream)
    L = 6 if a.mix == "full" else a.lights
    points_needed = {"spots": 0, "point": 1, "full": 2}[a.mix]
    owned, lights, origins = [], [], []
    for k in range(points_needed):
        light = srt.OmniLight(path, 0, POINTS[k])
        light.prepare(a.face, stream)
        owned.append(light)
        origins.append(POINTS[k])
        lights.append(srt.PointLight(light, COLORS[len(lights)], falloff=1.0, bias=a.bias))
    for k in range(L - points_needed):
        scene = srt.DeviceScene(path, 0, camera=spot_camera(k))
        scene.prepare(a.spot, a.spot, stream)
        owned.append(scene)
        origins.append(spot_camera(k)[:3])
        lights.append(srt.SpotLight(scene, COLORS[len(lights)], falloff=4.0, bias=a.bias))
    origins = [torch.tensor(o, **f32) for o in origins]
    colors = [torch.tensor(l.color, **f32) for l in lights]
    gen = torch.Generator(device=dev).manual_seed(7)
    normals = torch.rand((n, 3, 3), generator=gen, **f32) * 2 - 1
    uvs = torch.rand((n, 3, 2), generator=gen, **f32) * 4 - 1.5
    material = srt.Material((0.9, 0.7, 0.5), 5)

    eye, base, du, dv = (torch.tensor(v, **f32) for v in scene_frame(path, W, H))
    fx = ((torch.arange(W, **f32) + 0.5) / W)[None, :, None]
    fy = ((torch.arange(H, **f32) + 0.5) / H)[:, None, None]
    d = (base + fx * du) + fy * dv
    rgba, other, crgba, normal, albedo, gnormal = (torch.empty((H, W, 4), **f32) for _ in range(6))
    depth = torch.empty((H, W), **f32)
    classes = torch.empty((L, H, W), dtype=torch.uint8, device=dev)
    masks = torch.empty((L, H, W), dtype=torch.uint8, device=dev)
    amb = torch.tensor(AMBIENT, **f32)

    for T in a.texture:
        tex = torch.rand((T, T, 4), generator=gen, **f32)
        surface = srt.Surface(normals, uvs, tex)

        def composition():
            view.light(lights, off, ids, other, ambient=AMBIENT, classes=masks, stream=stream)
            view.surface_frame(off, ids, surface, normal=normal, albedo=albedo, stream=stream)
            view.gbuffer(off, ids, depth=depth, normal=gnormal, stream=stream)
            u, n3 = normal[..., :3], gnormal[..., :3]
            p = eye + depth[..., None] * d
            nd = (n3 * d).sum(-1)
            e = amb.expand(H, W, 3).clone()
            for k, l in enumerate(lights):
                q = p - origins[k]
                qq = (q * q).sum(-1)
                w = (-(u * q).sum(-1) / qq.sqrt()).clamp(0.0, 1.0) * (l.falloff / qq)
                on = (masks[k] == 1) & ((n3 * q).sum(-1) * nd > 0)
                e += torch.where(on, w, torch.zeros_like(w))[..., None] * colors[k]
            crgba[..., :3] = albedo[..., :3] * e
            crgba[..., 3] = albedo[..., 3]

        def back_to_back():
            view.light(lights, off, ids, other, ambient=AMBIENT, stream=stream)
            view.surface_frame(off, ids, surface, normal=normal, albedo=albedo, stream=stream)

        cases = {
            "fused": lambda: view.light_surface(lights, off, ids, surface, rgba, ambient=AMBIENT, stream=stream),
            "fused_classes": lambda: view.light_surface(lights, off, ids, surface, rgba, ambient=AMBIENT, classes=classes,
                                                        stream=stream),
            "fused_specular": lambda: view.light_surface(lights, off, ids, surface, other, ambient=AMBIENT,
                                                         material=material, stream=stream),
            "bare": lambda: view.light_surface(lights, off, ids, None, other, ambient=AMBIENT, stream=stream),
            "lighting": lambda: view.light(lights, off, ids, other, ambient=AMBIENT, stream=stream),
            "surface": lambda: view.surface_frame(off, ids, surface, normal=normal, albedo=albedo, stream=stream),
            "back_to_back": back_to_back,
            "composition": composition,
        }
        # The answers first (and a warm-up launch of each shape: builds the setups).
        cases["bare"]()
        bare = other.clone()
        cases["lighting"]()
        torch.cuda.synchronize()
        if not torch.equal(bare.view(torch.int32), other.view(torch.int32)):
            raise SystemExit("the fused call without surface and material differs from rtdLightAsync")
        for run in cases.values():
            run()
        cases["fused_classes"]()
        torch.cuda.synchronize()
        if not torch.equal(classes, masks):
            raise SystemExit("the fused call's class planes differ from rtdLightAsync's")
        hit = ids >= 0
        rgb_err = float((rgba[..., :3] - crgba[..., :3])[hit].abs().max().item())

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
        out = {"library": a.child, "mix": a.mix, "lights": L, "workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5",
               "texture": f"{T}x{T} ({T * T * 16 // 1024} KB)", "spot_size": a.spot, "face_size": a.face,
               "hits": int(hit.sum().item()), "launches": a.launches, "repeats": a.repeats,
               "device": torch.cuda.get_device_name(0), "rgb_max_abs_vs_composition": rgb_err, "cases": {}}
        for name, v in us.items():
            out["cases"][name] = {"us_per_launch": round(statistics.median(v), 1), "us_min": round(min(v), 1),
                                  "us_max": round(max(v), 1)}
        c = out["cases"]
        out["fused_over_back_to_back"] = round(c["fused"]["us_per_launch"] / c["back_to_back"]["us_per_launch"], 3)
        out["fused_over_composition"] = round(c["fused"]["us_per_launch"] / c["composition"]["us_per_launch"], 3)
        out["bare_over_lighting"] = round(c["bare"]["us_per_launch"] / c["lighting"]["us_per_launch"], 3)
        out["fused_beats_back_to_back"] = c["fused"]["us_max"] < c["back_to_back"]["us_min"]
        print(json.dumps(out), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"probe_{a.child}_{a.mix}{L}_t{T}.json"), "w") as f:
                json.dump(out, f, indent=1)
    for o in owned:
        o.close()
    view.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", choices=("spots", "point", "full"), default="point")
    ap.add_argument("--lights", type=int, default=4)
    ap.add_argument("--texture", default="64,1024", help="texels per side, one run per value")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spot", type=int, default=1024, help="the spot lights' frames are SPOT x SPOT")
    ap.add_argument("--face", type=int, default=512, help="the cube faces are FACE x FACE")
    ap.add_argument("--bias", type=float, default=2.0 ** -10)
    ap.add_argument("--out", default=None, help="directory for one JSON per library, mix and texture")
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="a library to measure (SRT_LIB)")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        a.texture = [int(v) for v in a.texture.split(",")]
        step(a)
        return
    libs = [s.split("=", 1) for s in a.lib] or [["product", ""]]
    for name, lib in libs:
        env = dict(os.environ)
        if lib:
            env["SRT_LIB"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", name]
        for key in ("mix", "lights", "texture", "launches", "repeats", "triangles", "width", "height", "spot", "face", "bias"):
            cmd += [f"--{key}", str(getattr(a, key))]
        cmd += ["--out", a.out] if a.out else []
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:  # nothing more is started after a step that failed, faulted or timed out
            raise SystemExit(f"step {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
