#!/usr/bin/env python3
"""Ray-query throughput: the world-space tree against brute force, beside the cull trace (run on the GPU box).

    python tools/rays_probe.py [--launches 5] [--repeats 3] [--triangles 100000] [--subset 32768] [--out FILE]

C3 (soup-100k, 1920 x 1080, offsets 0.5) in one process, one scene, one stream. Two ray sets of
2 073 600 rays each:

    camera   the frame's pixels as rays (device.camera_rays): coherent, one origin
    random   origins uniform in the scene's bounds, random directions: incoherent

Each is timed for closest hit and for occlusion on the tree (SRT_RAYS=tree, the default) and, on
the first --subset rays of a shuffled copy of the set, on the brute-force kernel (SRT_RAYS=brute);
next to them the cull trace's ids of the same frame (srtTraceIdsAsync). Every case is timed with
device events around --launches launches after a warm-up launch, the cases alternated within every
repeat. Reports Mrays/s and us per launch (median over the repeats, with min and max), the
tree-over-brute ratio per set, the tree's build time and the share of camera rays whose id is the
trace's (they are not bit-equal by design). Before anything is timed, the tree's answers on the
subset are checked against the brute-force kernel's, bit for bit.
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
    ap.add_argument("--subset", type=int, default=32768, help="rays of each set given to the brute-force kernel")
    ap.add_argument("--out", default=None, help="also write the summary JSON here")
    a = ap.parse_args()
    import numpy as np
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd import device

    W, H = a.width, a.height
    count = W * H
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    scene = srt.DeviceScene(path, 0)
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    off = torch.full((H, W, 2), 0.5, dtype=torch.float32, device=dev)
    frame = torch.empty((H, W), dtype=torch.int32, device=dev)

    rng = np.random.default_rng(1)
    v = device.read_scene(path)["vertices"].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    random = np.empty((count, 8), np.float32)
    random[:, 0:3] = rng.uniform(lo, hi, (count, 3))
    random[:, 3] = 0.0
    random[:, 4:7] = rng.normal(size=(count, 3))
    random[:, 7] = np.inf
    sets_np = {"camera": device.camera_rays(path, W, H, 0.5), "random": random}
    sets, subsets = {}, {}
    for name, r in sets_np.items():
        sets[name] = torch.from_numpy(r).to(dev)
        subsets[name] = torch.from_numpy(np.ascontiguousarray(r[rng.permutation(count)[:a.subset]])).to(dev)
    ids = torch.empty((count,), dtype=torch.int32, device=dev)
    t = torch.empty((count,), dtype=torch.float32, device=dev)
    occ = torch.empty((count,), dtype=torch.uint8, device=dev)
    sub = a.subset

    def run(kind, rays, n, mode):
        os.environ["SRT_RAYS"] = mode
        if kind == "closest":
            scene.closest(rays, ids[:n], t[:n], stream=stream)
        else:
            scene.occluded(rays, occ[:n], stream=stream)

    # The build, timed on its own; then the tree against the brute-force kernel on the subsets.
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    scene.build_rays(stream)
    e1.record(stream)
    e1.synchronize()
    build_ms = e0.elapsed_time(e1)
    for name in sets:
        run("closest", subsets[name], sub, "tree")
        run("occluded", subsets[name], sub, "tree")
        torch.cuda.synchronize()
        want = (ids[:sub].clone(), t[:sub].clone(), occ[:sub].clone())
        run("closest", subsets[name], sub, "brute")
        run("occluded", subsets[name], sub, "brute")
        torch.cuda.synchronize()
        if not (torch.equal(ids[:sub], want[0]) and torch.equal(t[:sub].view(torch.int32), want[1].view(torch.int32))
                and torch.equal(occ[:sub], want[2])):
            raise SystemExit(f"{name}: the tree's answers differ from the brute-force kernel's")
    scene.trace_ids(off, frame, 0, H, variant="cull", stream=stream)
    run("closest", sets["camera"], count, "tree")
    torch.cuda.synchronize()
    same_as_trace = float((ids == frame.reshape(-1)).float().mean().item())
    hit_share = {}
    for name in sets:
        run("occluded", sets[name], count, "tree")
        torch.cuda.synchronize()
        hit_share[name] = round(float(occ.float().mean().item()), 4)

    cases = {"trace_cull": (count, lambda: scene.trace_ids(off, frame, 0, H, variant="cull", stream=stream))}
    for name in sets:
        for kind in ("closest", "occluded"):
            cases[f"{kind}_{name}_tree"] = (count, lambda k=kind, s=name: run(k, sets[s], count, "tree"))
            cases[f"{kind}_{name}_brute"] = (sub, lambda k=kind, s=name: run(k, subsets[s], sub, "brute"))
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
    os.environ.pop("SRT_RAYS", None)
    out = {"workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5", "rays_per_set": count, "brute_subset": sub,
           "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "tree_build_ms": round(build_ms, 3), "camera_ids_equal_to_trace": round(same_as_trace, 6),
           "occluded_share": hit_share, "cases": {}, "tree_over_brute": {}}
    for name, v_us in us.items():
        med = statistics.median(v_us)
        out["cases"][name] = {"rays": cases[name][0], "us_per_launch": round(med, 1), "us_min": round(min(v_us), 1),
                              "us_max": round(max(v_us), 1), "mrays_per_s": round(cases[name][0] / med, 1)}
        print(json.dumps({name: out["cases"][name]}), flush=True)
    for name in sets:
        for kind in ("closest", "occluded"):
            tree, brute = out["cases"][f"{kind}_{name}_tree"], out["cases"][f"{kind}_{name}_brute"]
            out["tree_over_brute"][f"{kind}_{name}"] = round(tree["mrays_per_s"] / brute["mrays_per_s"], 1)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    scene.close()


if __name__ == "__main__":
    main()
