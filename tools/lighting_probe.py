#!/usr/bin/env python3
"""Direct-lighting time against the composition of the calls that existed before it (run on the GPU box).

    python tools/lighting_probe.py --mix spots|point|full [--lights 1,2,4,8] [--spot 1024] [--face 512]
                                   [--launches 20] [--repeats 5] [--out FILE]

C3 (soup-100k, 1920 x 1080, offsets 0.5) in one process, one stream. The soup fills [-1, 1] x [-1, 1]
x [2, 4]. Spot lights stand on a ring of radius 3 around its centre, 2.5 above it, looking at the
centre (vfov 50 degrees, --spot x --spot frames); the point lights sit inside the soup at (0.1, 0.2,
3.0) and (-0.4, -0.1, 2.6) with --face x --face cube faces. The hit ids are the view's own cull trace.
Mixes, for every L of --lights:

    spots   L spot lights
    point   one point light inside the soup and L - 1 spot lights
    full    two point lights and four spot lights (L = 6, 16 light frames; --lights is ignored)

Four cases per L, alternated within every repeat, each timed with device events around --launches
launches after a warm-up launch of each shape:

    fused           rtdLightAsync, RGBA only
    fused_classes   rtdLightAsync, RGBA and the L class planes
    shadows         the L single-light launches the fused call replaces (rtlShadowAsync /
                    rtoShadowAsync into L mask planes) and nothing else
    composition     those L launches, rtgFrameAsync (normal, albedo, depth), and in torch the surface
                    point P = eye + depth d, then per light q, the two cosines' signs, the weight and
                    the accumulation, and albedo . E (d, a constant of the frame, is computed outside
                    the timed region)

Before timing, the L class planes of the fused call are compared with the single-light masks on every
pixel (the probe refuses to go on if one differs) and the fused RGBA with the composition's (the
largest difference is reported: the composition's arithmetic is torch's, not the definition's).
Reports, per case, us per launch (median over the repeats) and the spread (min, max), and whether the
fused call took no longer than the `shadows` sum. No speed-up is asserted.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

POINTS = ((0.1, 0.2, 3.0), (-0.4, -0.1, 2.6))
COLORS = ((1.0, 0.9, 0.8), (0.3, 0.6, 1.0), (0.9, 0.3, 0.2), (0.2, 0.8, 0.3), (0.7, 0.7, 0.1), (0.5, 0.2, 0.9),
          (0.1, 0.6, 0.6), (0.8, 0.8, 0.8))
AMBIENT = (0.05, 0.05, 0.05)


def spot_camera(k: int):
    a = 2.0 * math.pi * (k + 0.25) / 8.0
    return (3.0 * math.cos(a), 2.5, 3.0 + 3.0 * math.sin(a), 0.0, 0.0, 3.0, 0.0, 1.0, 0.0, 50.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", choices=("spots", "point", "full"), default="spots")
    ap.add_argument("--lights", default="1,2,4,8")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spot", type=int, default=1024, help="the spot lights' frames are SPOT x SPOT")
    ap.add_argument("--face", type=int, default=512, help="the cube faces are FACE x FACE")
    ap.add_argument("--bias", type=float, default=2.0 ** -10)
    ap.add_argument("--out", default=None, help="also write the summary JSON here")
    a = ap.parse_args()
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.device import scene_frame

    W, H = a.width, a.height
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    stream = torch.cuda.current_stream()
    view = srt.DeviceScene(path, 0)
    view.prepare(W, H, stream)
    off = torch.full((H, W, 2), 0.5, dtype=torch.float32, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    view.trace_ids(off, ids, 0, H, variant="cull", stream=stream)
    counts = [int(v) for v in a.lights.split(",")] if a.mix != "full" else [6]
    points_needed = {"spots": 0, "point": 1, "full": 2}[a.mix]
    spots_needed = 4 if a.mix == "full" else max(counts) - points_needed
    owned = []
    pool = []
    for k in range(points_needed):
        light = srt.OmniLight(path, 0, POINTS[k])
        light.prepare(a.face, stream)
        owned.append(light)
        pool.append(srt.PointLight(light, COLORS[len(pool)], falloff=1.0, bias=a.bias))
    for k in range(spots_needed):
        scene = srt.DeviceScene(path, 0, camera=spot_camera(k))
        scene.prepare(a.spot, a.spot, stream)
        owned.append(scene)
        pool.append(srt.SpotLight(scene, COLORS[len(pool)], falloff=4.0, bias=a.bias))

    # the frame's constants for the torch side of the composition
    eye, base, du, dv = (torch.tensor(v, dtype=torch.float32, device=dev) for v in scene_frame(path, W, H))
    fx = ((torch.arange(W, dtype=torch.float32, device=dev) + 0.5) / W)[None, :, None]
    fy = ((torch.arange(H, dtype=torch.float32, device=dev) + 0.5) / H)[:, None, None]
    d = (base + fx * du) + fy * dv
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    crgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    normal = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    albedo = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    amb = torch.tensor(AMBIENT, dtype=torch.float32, device=dev)

    results = []
    for L in counts:
        lights = pool[:L]
        frames = sum(6 if isinstance(l, srt.PointLight) else 1 for l in lights)
        classes = torch.empty((L, H, W), dtype=torch.uint8, device=dev)
        masks = torch.empty((L, H, W), dtype=torch.uint8, device=dev)
        origins = [torch.tensor(l.light.origin if isinstance(l, srt.PointLight) else spot_camera(pool.index(l) - points_needed)[:3],
                                dtype=torch.float32, device=dev) for l in lights]
        colors = [torch.tensor(l.color, dtype=torch.float32, device=dev) for l in lights]

        def shadows():
            for k, l in enumerate(lights):
                if isinstance(l, srt.PointLight):
                    view.omni_shadow(l.light, off, ids, masks[k], bias=l.bias, stream=stream)
                else:
                    view.shadow(l.scene, off, ids, masks[k], None, bias=l.bias, stream=stream)

        def composition():
            shadows()
            view.gbuffer(off, ids, depth=depth, normal=normal, albedo=albedo, stream=stream)
            n3 = normal[..., :3]
            p = eye + depth[..., None] * d
            nd = (n3 * d).sum(-1)
            nn = (n3 * n3).sum(-1)
            e = amb.expand(H, W, 3).clone()
            for k, l in enumerate(lights):
                q = p - origins[k]
                nl = (n3 * q).sum(-1)
                qq = (q * q).sum(-1)
                w = (nl.abs() / (nn.sqrt() * qq.sqrt())).clamp(max=1.0) * (l.falloff / qq)
                on = (masks[k] == 1) & (nl * nd > 0)
                e += torch.where(on, w, torch.zeros_like(w))[..., None] * colors[k]
            crgba[..., :3] = albedo[..., :3] * e
            crgba[..., 3] = albedo[..., 3]

        cases = {
            "fused": lambda: view.light(lights, off, ids, rgba, ambient=AMBIENT, stream=stream),
            "fused_classes": lambda: view.light(lights, off, ids, rgba, ambient=AMBIENT, classes=classes, stream=stream),
            "shadows": shadows,
            "composition": composition,
        }
        for run in cases.values():  # warm-up: builds the setups, checks below
            run()
        torch.cuda.synchronize()
        differ = [int((classes[k] != masks[k]).sum().item()) for k in range(L)]
        if any(differ):
            raise SystemExit(f"L = {L}: class planes differ from the single-light masks: {differ}")
        surface = ids >= 0
        rgb_err = float((rgba[..., :3] - crgba[..., :3])[surface].abs().max().item())
        with_classes = rgba.clone()
        cases["fused"]()
        torch.cuda.synchronize()
        if not torch.equal(with_classes.view(torch.int32), rgba.view(torch.int32)):
            raise SystemExit(f"L = {L}: the RGBA without class planes differs from the RGBA with them")
        class_counts = [[int((classes[k] == c).sum().item()) for c in range(4)] for k in range(L)]

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
        out = {"mix": a.mix, "lights": L, "light_frames": frames, "workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5",
               "spot_size": a.spot, "face_size": a.face, "bias": a.bias, "pixels_per_launch": W * H, "launches": a.launches,
               "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "lib": os.environ.get("SRT_LIB", "product"),
               "class_mismatches": differ, "class_counts": class_counts, "rgb_max_abs_vs_composition": rgb_err, "cases": {}}
        for name, v in us.items():
            med = statistics.median(v)
            out["cases"][name] = {"us_per_launch": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
        c = out["cases"]
        out["fused_over_shadows"] = round(c["fused"]["us_per_launch"] / c["shadows"]["us_per_launch"], 3)
        out["fused_over_composition"] = round(c["fused"]["us_per_launch"] / c["composition"]["us_per_launch"], 3)
        # the expectation: no longer than the sum of the L shadow launches, within the composition's own spread
        margin = c["composition"]["us_max"] - c["composition"]["us_min"]
        out["fused_within_shadows_sum"] = c["fused"]["us_per_launch"] <= c["shadows"]["us_per_launch"] + margin
        print(json.dumps(out), flush=True)
        results.append(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    for o in owned:
        o.close()
    view.close()


if __name__ == "__main__":
    main()
