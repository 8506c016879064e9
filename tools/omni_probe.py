#!/usr/bin/env python3
"""Omni-light shadow time against the composition of the calls that existed before it (run on the GPU box).

    python tools/omni_probe.py [--launches 20] [--repeats 5] [--face 512] [--light inside|outside] [--out FILE]

C3 (soup-100k, 1920 x 1080, offsets 0.5) in one process, one stream. The soup fills [-1, 1] x [-1, 1]
x [2, 4]; the point light sits inside it (0.1, 0.2, 3.0) or outside, above it (0, 4, 3), with cube
faces of --face x --face (default 512). The hit ids are the view's own cull trace. Three cases,
alternated within every repeat, each timed with device events around --launches launches after a
warm-up launch of each shape:

    omni_mask        rtoShadowAsync, mask only
    omni_mask_face   rtoShadowAsync, mask and face plane
    composition      six rtlShadowAsync launches over the whole band on six DeviceScene(path,
                     camera=face camera) scenes prepared at the face size, into the planes of one
                     (6, H, W) tensor, and a torch.gather by the face plane. The face plane is taken as
                     given (the fused call's, converted to gather's int64 index outside the timed
                     region): the composition is not charged for choosing faces.

Before timing, the fused mask is checked against the composition's on every pixel, none of the
selected classes may be 2, and the class counts and pixels per face are printed. Also reported: the
wall time of OmniLight() (six scene loads and spatial orders) and the device memory the light holds
after its first call (six copies of the vertices, orders, records and setups), beside one
DeviceScene's. Reports, per case, us per launch (median over the repeats), the spread (min, max) and
the ratio fused / composition. No speed-up is asserted.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIGHTS = {"inside": (0.1, 0.2, 3.0), "outside": (0.0, 4.0, 3.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--face", type=int, default=512, help="the cube faces are FACE x FACE")
    ap.add_argument("--light", choices=sorted(LIGHTS), default="inside")
    ap.add_argument("--bias", type=float, default=0.0)
    ap.add_argument("--out", default=None, help="also write the summary JSON here")
    a = ap.parse_args()
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.device import omni_face_camera

    W, H, F = a.width, a.height, a.face
    origin = LIGHTS[a.light]
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    stream = torch.cuda.current_stream()

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    m0 = used()
    view = srt.DeviceScene(path, 0)
    view.prepare(W, H, stream)
    off = torch.full((H, W, 2), 0.5, dtype=torch.float32, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    view.trace_ids(off, ids, 0, H, variant="cull", stream=stream)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    face = torch.empty((H, W), dtype=torch.uint8, device=dev)
    planes = torch.empty((6, H, W), dtype=torch.uint8, device=dev)
    cmask = torch.empty((1, H, W), dtype=torch.uint8, device=dev)
    m1 = used()

    t0 = time.perf_counter()
    light = srt.OmniLight(path, 0, origin)
    torch.cuda.synchronize()
    create_ms = (time.perf_counter() - t0) * 1e3
    light.prepare(F, stream)
    view.omni_shadow(light, off, ids, mask, face, bias=a.bias, stream=stream)  # builds the six setups
    m2 = used()

    spots = [srt.DeviceScene(path, 0, camera=omni_face_camera(origin, k)) for k in range(6)]
    for s in spots:
        s.prepare(F, F, stream)
    index = face.clamp(max=5).to(torch.int64)[None]  # (a class-3 pixel is class 3 under every face)

    def composition():
        for k in range(6):
            view.shadow(spots[k], off, ids, planes[k], None, bias=a.bias, stream=stream)
        torch.gather(planes, 0, index, out=cmask)

    cases = {
        "omni_mask": lambda: view.omni_shadow(light, off, ids, mask, None, bias=a.bias, stream=stream),
        "omni_mask_face": lambda: view.omni_shadow(light, off, ids, mask, face, bias=a.bias, stream=stream),
        "composition": composition,
    }
    composition()
    torch.cuda.synchronize()
    mismatches = {}
    for name in ("omni_mask", "omni_mask_face"):
        mask.fill_(9)
        cases[name]()
        torch.cuda.synchronize()
        mismatches[name] = int((mask != cmask[0]).sum().item())
        if mismatches[name]:
            raise SystemExit(f"{name}: {mismatches[name]} pixels differ from the composition's mask")
    counts = [int((mask == k).sum().item()) for k in range(4)]
    per_face = [int((face == k).sum().item()) for k in range(6)]
    if counts[2]:
        raise SystemExit(f"{counts[2]} pixels are outside their selected face's frustum")
    print(json.dumps({"class_counts": dict(zip(("shadowed", "lit", "outside", "no_surface"), counts)),
                      "pixels_per_face": per_face}), flush=True)

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
    out = {"workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5", "light": a.light, "origin": list(origin),
           "face_size": F, "bias": a.bias, "pixels_per_launch": W * H, "launches": a.launches, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "lib": os.environ.get("SRT_LIB", "product"),
           "class_counts": counts, "pixels_per_face": per_face, "mask_mismatches": mismatches,
           "light_create_ms": round(create_ms, 1), "light_device_mib": round((m2 - m1) / 2 ** 20, 1),
           "view_scene_and_buffers_mib": round((m1 - m0) / 2 ** 20, 1), "cases": {}}
    for name, v in us.items():
        med = statistics.median(v)
        out["cases"][name] = {"us_per_launch": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                              "mpixels_per_s": round(W * H / med, 1)}
    comp = out["cases"]["composition"]["us_per_launch"]
    for name in ("omni_mask", "omni_mask_face"):
        out["cases"][name]["fused_over_composition"] = round(out["cases"][name]["us_per_launch"] / comp, 3)
    out["fused_beats_composition"] = all(out["cases"][k]["us_max"] < out["cases"]["composition"]["us_min"]
                                         for k in ("omni_mask", "omni_mask_face"))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    light.close()
    for s in [view] + spots:
        s.close()


if __name__ == "__main__":
    main()
