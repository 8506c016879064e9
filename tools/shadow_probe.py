#!/usr/bin/env python3
"""Shadow-mask time against the composition of the calls that existed before it (run on the GPU box).

    python tools/shadow_probe.py [--launches 20] [--repeats 5] [--light 2048] [--light-camera above|eye] [--out FILE]

C3 (soup-100k, 1920 x 1080, offsets 0.5) in one process, one stream. The light is a spot above the
soup looking down into it: eye (0, 4, 3), lookat (0, 0, 3), up (0, 0, 1), vfov 45 degrees, a light
frame of --light x --light (default 2048 x 2048); --light-camera eye puts it at the view's eye
instead (every hit lit: no scan ends early). The hit ids are the view's own cull trace. Three
cases, alternated within every repeat, each timed with device events around --launches launches
after a warm-up launch of each shape:

    shadow_mask        rtlShadowAsync, mask only
    shadow_mask_rgba   rtlShadowAsync, mask and RGBA
    composition        the same mask from rtgFrameAsync (depth), the projection in torch (float32, one
                       op per step of DESIGN.md section 2 "Shadow"), rtqQueryAsync on a scene created
                       from a file with the light's camera, and a torch compare. Pixels that are not
                       in the light's frustum query position (0, 0), so that no query streams.

Before timing, the fused mask is checked against the composition's on every pixel and the class
counts are printed. Reports, per case, us per launch (median over the repeats) and the spread (min,
max). The sanity condition: both fused cases beat the composition measured in this very call.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import struct
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIGHT_CAMS = {
    "above": (0.0, 4.0, 3.0, 0.0, 0.0, 3.0, 0.0, 0.0, 1.0, 45.0),  # most surface pixels shadowed: scans end early
    "eye": (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 60.0),    # the soup's own camera: every hit lit, full scans
}
CAMERA_AT = 24  # byte offset of the 10 camera floats in a scene file's header (DESIGN.md "Scene file")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--light", type=int, default=2048, help="the light frame is LIGHT x LIGHT")
    ap.add_argument("--light-camera", choices=sorted(LIGHT_CAMS), default="above")
    ap.add_argument("--bias", type=float, default=0.0)
    ap.add_argument("--keep-going", action="store_true", help="time the cases even if the masks differ (reported)")
    ap.add_argument("--out", default=None, help="also write the summary JSON here")
    a = ap.parse_args()
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.device import light_projection, pixel_positions, scene_frame, shadow_host

    W, H, WL = a.width, a.height, a.light
    LIGHT_CAM = LIGHT_CAMS[a.light_camera]
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    light_path = os.path.join(tmp.name, "light.srt")
    with open(path, "rb") as f:
        blob = bytearray(f.read())
    blob[CAMERA_AT:CAMERA_AT + 40] = struct.pack("<10f", *LIGHT_CAM)
    with open(light_path, "wb") as f:
        f.write(blob)
    stream = torch.cuda.current_stream()
    view = srt.DeviceScene(path, 0)
    light = srt.DeviceScene(path, 0, camera=LIGHT_CAM)  # the fused call's light
    light_file = srt.DeviceScene(light_path, 0)         # the composition's: what existed before
    view.prepare(W, H, stream)
    light.prepare(WL, WL, stream)
    light_file.prepare(WL, WL, stream)
    off = torch.full((H, W, 2), 0.5, dtype=torch.float32, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    view.trace_ids(off, ids, 0, H, variant="cull", stream=stream)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)

    # The composition's constants: the view frame, ray generation's positions, the light's rows.
    eye, base, du, dv = (torch.tensor(v, dtype=torch.float32, device=dev) for v in scene_frame(path, W, H))
    lorigin = torch.tensor(LIGHT_CAM[0:3], dtype=torch.float32, device=dev)
    px, py, pz = (torch.from_numpy(r).to(dev) for r in light_projection(LIGHT_CAM, WL, WL))
    # (numpy's correctly rounded division: torch divides by a host scalar through its reciprocal)
    fxy = torch.from_numpy(pixel_positions(W, H, 0.5).reshape(H, W, 2)).to(dev)
    fx, fy = fxy[..., 0].contiguous(), fxy[..., 1].contiguous()
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    qid = torch.empty((H * W,), dtype=torch.int32, device=dev)
    qt = torch.empty((H * W,), dtype=torch.float32, device=dev)
    bias = torch.tensor(a.bias, dtype=torch.float32, device=dev)
    n = view.triangles
    cmask = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def dotp(q, r):
        return (q[0] * r[0] + q[1] * r[1]) + q[2] * r[2]

    def composition():
        view.gbuffer(off, ids, depth=depth, stream=stream)
        q = [(eye[k] + depth * ((base[k] + fx * du[k]) + fy * dv[k])) - lorigin[k] for k in range(3)]
        z = dotp(q, pz)
        gx, gy = dotp(q, px) / z, dotp(q, py) / z
        surface = (ids >= 0) & (ids < n)
        inside = surface & (z > 0) & (z < float("inf")) & (gx >= 0) & (gx <= 1) & (gy >= 0) & (gy <= 1)
        pos = torch.stack([torch.where(inside, gx, 0.0), torch.where(inside, gy, 0.0)], dim=-1).reshape(-1, 2)
        light_file.query(pos, qid, qt, stream=stream)
        thr = z - bias * z
        lit = (qid.reshape(H, W) == ids) | (qt.reshape(H, W) >= thr)
        cls = torch.where(lit, 1, 0)
        cls = torch.where(inside, cls, 2)
        cmask.copy_(torch.where(surface, cls, 3))

    cases = {
        "shadow_mask": lambda: view.shadow(light, off, ids, mask, None, bias=a.bias, dim=0.25, stream=stream),
        "shadow_mask_rgba": lambda: view.shadow(light, off, ids, mask, rgba, bias=a.bias, dim=0.25, stream=stream),
        "composition": composition,
    }
    # Warm-up launch of each shape, and the masks compared while at it.
    composition()
    torch.cuda.synchronize()
    mismatches = {}
    for name in ("shadow_mask", "shadow_mask_rgba"):
        mask.fill_(9)
        cases[name]()
        torch.cuda.synchronize()
        differ = int((mask != cmask).sum().item())
        if differ:
            # Which side is off: the host's brute-force answer for the first rows that differ.
            rows_off = sorted({int(i) // W for i in torch.nonzero((mask != cmask).reshape(-1))[:, 0].tolist()})[:4]
            for y in rows_off:
                hm, _ = shadow_host(path, W, H, LIGHT_CAM, WL, WL, off[y:y + 1].cpu().numpy(),
                                    ids[y:y + 1].cpu().numpy(), bias=a.bias, row_begin=y, row_count=1)
                hm = torch.from_numpy(hm[0]).to(dev)
                xs = torch.nonzero(mask[y] != cmask[y])[:, 0].tolist()
                print(json.dumps({"row": y, "columns": xs, "fused": mask[y][xs].tolist(), "composition": cmask[y][xs].tolist(),
                                  "host": hm[xs].tolist(), "fused_row_equals_host": bool(torch.equal(mask[y], hm))}),
                      flush=True)
            if not a.keep_going:
                raise SystemExit(f"{name}: {differ} pixels differ from the composition's mask")
        mismatches[name] = differ
    counts = [int((mask == k).sum().item()) for k in range(4)]
    print(json.dumps({"class_counts": dict(zip(("shadowed", "lit", "outside", "no_surface"), counts))}), flush=True)

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
    out = {"workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5", "light_camera": list(LIGHT_CAM),
           "light_frame": [WL, WL], "bias": a.bias, "pixels_per_launch": W * H, "launches": a.launches,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "lib": os.environ.get("SRT_LIB", "product"),
           "class_counts": counts, "mask_mismatches": mismatches, "cases": {}}
    for name, v in us.items():
        med = statistics.median(v)
        out["cases"][name] = {"us_per_launch": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                              "mpixels_per_s": round(W * H / med, 1)}
        print(json.dumps({name: out["cases"][name]}), flush=True)
    comp = out["cases"]["composition"]["us_min"]
    out["fused_beats_composition"] = all(out["cases"][k]["us_max"] < comp for k in ("shadow_mask", "shadow_mask_rgba"))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    for s in (view, light, light_file):
        s.close()
    if not out["fused_beats_composition"]:
        raise SystemExit("sanity condition failed: a fused case is not faster than the composition")


if __name__ == "__main__":
    main()
