#!/usr/bin/env python3
"""Sampled radiance, the fused call against the composition it replaces (run on the GPU box).

    python tools/radiance_probe.py [--samples 1,4,16] [--width 1920] [--height 1080] [--triangles 100000]
                                   [--launches 5] [--repeats 3] [--small 2000] [--out FILE]

Two scenes at --width x --height, offsets 0.5, under one point light and three spot lights: C3
(soup-100k, the lights of tools/lighting_probe.py) and the Cornell box. The hit ids are the view's own
cull trace. Per S of --samples, with and without the rotation table, two cases alternated within
every repeat, each timed with device events around --launches launches after a warm-up launch:

    fused        scene.radiance_frame: one launch, no scratch
    composition  generate_rays_frame -> closest -> light_hits -> the sum over s in ascending order
                 and the divide (torch, on the device): S x elements x 56 bytes of scratch

Before timing, the two are compared on every bit (the probe refuses to go on if one differs). On a
small scene (soup of --small triangles at 320 x 180, S = 4) the tree is timed against SRT_RAYS=brute.
Reports, per case, us per launch (median over the repeats), the spread (min, max) and the
composition's scratch bytes beside the fused call's zero. No threshold is asserted.
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
sys.path.insert(0, os.path.join(REPO, "tools"))

CORNELL_SPOTS = ((0.4, 1.2, 0.6, 0.0, 0.6, 2.7, 0.0, 1.0, 0.0, 70.0), (-0.4, 1.0, 0.5, 0.2, 0.4, 2.7, 0.0, 1.0, 0.0, 70.0),
                 (0.0, 0.3, 0.4, 0.0, 1.0, 2.7, 0.0, 1.0, 0.0, 70.0))
CORNELL_POINT = (0.0, 1.0, 2.7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="1,4,16")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--small", type=int, default=2000, help="triangles of the tree-against-brute scene")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spot", type=int, default=1024, help="the spot lights' frames are SPOT x SPOT")
    ap.add_argument("--face", type=int, default=512, help="the cube faces are FACE x FACE")
    ap.add_argument("--bias", type=float, default=2.0 ** -10)
    ap.add_argument("--out", default=None, help="also write the summary JSON here")
    a = ap.parse_args()
    import torch

    import simpleraytracer_amd as srt
    from lighting_probe import AMBIENT, COLORS, POINTS, spot_camera
    from simpleraytracer_amd import samples as sm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    tmp = tempfile.TemporaryDirectory()

    def timed(cases, launches, repeats):
        us = {name: [] for name in cases}
        for _ in range(repeats):
            for name, run in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _k in range(launches):
                    run()
                e1.record(stream)
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / launches)
        return {name: {"us_per_launch": round(statistics.median(v), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
                for name, v in us.items()}

    class Workload:
        def __init__(self, path, w, h, spots, point):
            self.w, self.h = w, h
            self.view = srt.DeviceScene(path, 0)
            self.view.prepare(w, h, stream)
            self.off = torch.full((h, w, 2), 0.5, dtype=torch.float32, device=dev)
            self.ids = torch.empty((h, w), dtype=torch.int32, device=dev)
            self.view.trace_ids(self.off, self.ids, 0, h, variant="cull", stream=stream)
            self.owned, self.lights = [], []
            light = srt.OmniLight(path, 0, point)
            light.prepare(a.face, stream)
            self.owned.append(light)
            self.lights.append(srt.PointLight(light, COLORS[0], falloff=1.0, bias=a.bias))
            for k, cam in enumerate(spots):
                scene = srt.DeviceScene(path, 0, camera=cam)
                scene.prepare(a.spot, a.spot, stream)
                self.owned.append(scene)
                self.lights.append(srt.SpotLight(scene, COLORS[1 + k], falloff=4.0, bias=a.bias))
            self.fused_out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
            self.composed_out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)

        def generator(self, S, rot):
            up = lambda t: torch.from_numpy(t).to(dev)  # noqa: E731
            return srt.Hemisphere(up(sm.cosine_hemisphere(S, 3)), 2.0 ** -10, float("inf"), up(sm.rotations(53)) if rot else None)

        def cases(self, S, rot):
            w, h, view = self.w, self.h, self.view
            gen = self.generator(S, rot)
            rays = torch.empty((S, h, w, 8), dtype=torch.float32, device=dev)
            hid = torch.empty((S * h * w,), dtype=torch.int32, device=dev)
            t = torch.empty((S * h * w,), dtype=torch.float32, device=dev)
            c = torch.empty((S * h * w, 4), dtype=torch.float32, device=dev)
            scratch = sum(x.numel() * x.element_size() for x in (rays, hid, t, c))
            fS = torch.tensor(float(S), dtype=torch.float32, device=dev)

            def fused():
                view.radiance_frame(self.lights, self.off, self.ids, gen, self.fused_out, ambient=AMBIENT, stream=stream)

            def composition():
                view.generate_rays_frame(self.off, self.ids, gen, rays, stream=stream)
                view.closest(rays.view(-1, 8), hid, t, stream=stream)
                view.light_hits(self.lights, rays.view(-1, 8), hid, t, c, ambient=AMBIENT, stream=stream)
                cs = c.view(S, h, w, 4)
                total = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
                for s in range(S):
                    total = total + cs[s, ..., :3]
                on = (rays[0, ..., 4:7] != 0).any(dim=-1)
                self.composed_out[..., :3] = torch.where(on[..., None], total / fS, torch.zeros_like(total))
                self.composed_out[..., 3] = torch.where(on, (cs[..., 3] >= 0).sum(dim=0).to(torch.float32) / fS,
                                                        torch.zeros_like(fS))

            return {"fused": fused, "composition": composition}, scratch

        def measure(self, S, rot, launches, repeats):
            cases, scratch = self.cases(S, rot)
            for run in cases.values():  # warm-up: builds the setups and the tree
                run()
            torch.cuda.synchronize()
            differ = int((self.fused_out.view(torch.int32) != self.composed_out.view(torch.int32)).sum().item())
            if differ:
                raise SystemExit(f"S = {S}, rotations {rot}: the fused call differs from the composition on {differ} values")
            out = timed(cases, launches, repeats)
            out.update(samples=S, rotations=rot, composition_scratch_bytes=scratch, fused_scratch_bytes=0,
                       fused_over_composition=round(out["fused"]["us_per_launch"] / out["composition"]["us_per_launch"], 3),
                       surface_elements=int((self.fused_out[..., 3] > 0).sum().item() + 0),
                       frame_surface=int((self.ids >= 0).sum().item()))
            return out

        def close(self):
            for o in self.owned:
                o.close()
            self.view.close()

    W, H = a.width, a.height
    report = {"workload": f"{W}x{H}, offsets 0.5, 1 point + 3 spot lights", "spot_size": a.spot, "face_size": a.face,
              "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
              "lib": os.environ.get("SRT_LIB", "product"), "scenes": {}}
    scenes = (("soup", srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles),
               [spot_camera(k) for k in range(3)], POINTS[0]),
              ("cornell", srt.write_scene(os.path.join(tmp.name, "cornell.srt"), "cornell"), CORNELL_SPOTS, CORNELL_POINT))
    for name, path, spots, point in scenes:
        wl = Workload(path, W, H, spots, point)
        rows = []
        for S in (int(v) for v in a.samples.split(",")):
            for rot in (False, True):
                rows.append(wl.measure(S, rot, a.launches, a.repeats))
                print(json.dumps({name: rows[-1]}), flush=True)
        report["scenes"][name] = rows
        wl.close()
    # tree against brute force, a small scene only
    small = Workload(srt.write_scene(os.path.join(tmp.name, "small.srt"), "soup", a.small), 320, 180,
                     [spot_camera(k) for k in range(3)], POINTS[0])
    modes = {}
    for mode in ("tree", "brute"):
        if mode == "brute":
            os.environ["SRT_RAYS"] = "brute"
        modes[mode] = small.measure(4, True, a.launches, a.repeats)
    os.environ.pop("SRT_RAYS", None)
    small.close()
    report["small"] = {"workload": f"soup-{a.small} 320x180, S = 4, rotations", **modes}
    print(json.dumps(report), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
