#!/usr/bin/env python3
"""Depth-layer throughput against the calls a caller would otherwise compose (run on the GPU box).

    python tools/layers_probe.py [--launches 10] [--repeats 5] [--triangles 100000] [--out FILE]

C3 (soup-100k, 1920 x 1080, offsets 0.5) in one process, one scene, one stream. Every case works on
the frame's 2 073 600 pixel positions; the cases are alternated within every repeat, each timed
with device events around --launches launches after a warm-up launch of each shape:

    query_{coherent,shuffled}       rtqQueryAsync, positions in row-major / random order
    query_x4_*, query_x8_*          4 / 8 back-to-back rtqQueryAsync calls: the list traffic a
                                    peel-by-passes design would pay (it would also need a lower bound)
    layers_k{1,4,8}_{coherent,shuffled}   rtkLayersAsync
    frame_k{1,4,8}                  rtkFrameAsync of the whole frame
    trace_lds                       srtTraceIdsAsync, lds variant: the brute-force floor
    composite_k{4,8}                rtkCompositeAsync of the frame's layers
    shade_x4, shade_x8              4 / 8 srtShadeAsync launches, one per id plane: the resolve's yardstick

Reports, per case, us per launch (median over the repeats) and the spread (min, max), and the
ratios the design discussion asks for. Layer 0 of every layers case is checked against the cull
trace's ids, and `how` against "no position streamed", before anything is timed.
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

KS = (1, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None, help="also write the summary JSON here")
    a = ap.parse_args()
    import numpy as np
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd.device import pixel_positions

    W, H = a.width, a.height
    rays = W * H
    dev = torch.device("cuda", 0)
    tmp = tempfile.TemporaryDirectory()
    path = srt.write_scene(os.path.join(tmp.name, "soup.srt"), "soup", a.triangles)
    scene = srt.DeviceScene(path, 0)
    stream = torch.cuda.current_stream()
    scene.prepare(W, H, stream)
    off = torch.full((H, W, 2), 0.5, dtype=torch.float32, device=dev)
    pos_np = pixel_positions(W, H, 0.5)
    perm = np.random.default_rng(1).permutation(rays)
    pos = {"coherent": torch.from_numpy(pos_np).to(dev),
           "shuffled": torch.from_numpy(np.ascontiguousarray(pos_np[perm])).to(dev)}
    ids = torch.empty((8, rays), dtype=torch.int32, device=dev)
    t = torch.empty((8, rays), dtype=torch.float32, device=dev)
    how = torch.empty((rays,), dtype=torch.uint8, device=dev)
    frame = torch.empty((H, W), dtype=torch.int32, device=dev)
    planes = torch.empty((8, H, W), dtype=torch.int32, device=dev)
    planes_t = torch.empty((8, H, W), dtype=torch.float32, device=dev)
    opacity = torch.full((scene.triangles,), 0.5, dtype=torch.float32, device=dev)
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)

    def queries(order, times):
        def run():
            for _ in range(times):
                scene.query(pos[order], ids[0], t[0], how, stream=stream)
        return run

    def shades(times):
        def run():
            for k in range(times):
                scene.shade(off, planes[k], rgba, stream=stream)
        return run

    cases = {}
    for order in ("coherent", "shuffled"):
        cases[f"query_{order}"] = queries(order, 1)
        cases[f"query_x4_{order}"] = queries(order, 4)
        cases[f"query_x8_{order}"] = queries(order, 8)
        for k in KS:
            cases[f"layers_k{k}_{order}"] = (lambda o=order, k=k: scene.layers(pos[o], ids[:k], t[:k], how, stream=stream))
    for k in KS:
        cases[f"frame_k{k}"] = lambda k=k: scene.layer_frame(off, planes[:k], planes_t[:k], stream=stream)
    cases["trace_lds"] = lambda: scene.trace_ids(off, frame, 0, H, variant="lds", stream=stream)
    for k in (4, 8):
        cases[f"composite_k{k}"] = lambda k=k: scene.composite(off, planes[:k], opacity, rgba, stream=stream)
        cases[f"shade_x{k}"] = shades(k)

    # The answers first: layer 0 is the cull trace's id, nothing streams, layers are prefixes.
    scene.trace_ids(off, frame, 0, H, variant="cull", stream=stream)
    torch.cuda.synchronize()
    want = frame.reshape(-1).clone()
    scene.layer_frame(off, planes, planes_t, stream=stream)  # the 8 planes the composite cases read
    torch.cuda.synchronize()
    if not torch.equal(planes[0], frame):
        raise SystemExit("frame_k8: layer 0 differs from the cull trace's ids")
    depth = {f"hits>={k}": int((planes[k - 1] >= 0).sum().item()) for k in (1, 2, 4, 8)}
    full = planes.reshape(8, -1).clone()
    for order in ("coherent", "shuffled"):
        index = None if order == "coherent" else torch.from_numpy(perm).to(dev)
        for k in KS:
            ids.fill_(-7)
            cases[f"layers_k{k}_{order}"]()
            torch.cuda.synchronize()
            expect = full[:k] if index is None else full[:k][:, index]
            if not torch.equal(ids[:k], expect):
                raise SystemExit(f"layers_k{k}_{order}: ids differ from the frame call's planes")
            if int((how != 0).sum().item()) != 0:
                raise SystemExit(f"layers_k{k}_{order}: positions streamed")
    if not torch.equal(full[0], want):
        raise SystemExit("layer 0 differs from the cull trace's ids")
    for run in cases.values():  # warm-up of every shape
        run()
    torch.cuda.synchronize()

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
    out = {"workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5", "positions_per_launch": rays,
           "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "lib": os.environ.get("SRT_LIB", "product"), "pixels_with": depth, "cases": {}}
    for name, v in us.items():
        med = statistics.median(v)
        out["cases"][name] = {"us": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
        print(json.dumps({name: out["cases"][name]}), flush=True)
    c = {k: v["us"] for k, v in out["cases"].items()}
    out["ratios"] = {}
    for order in ("coherent", "shuffled"):
        out["ratios"][f"layers_k1/query {order}"] = round(c[f"layers_k1_{order}"] / c[f"query_{order}"], 3)
        for k in (4, 8):
            out["ratios"][f"layers_k{k}/query_x{k} {order}"] = round(c[f"layers_k{k}_{order}"] / c[f"query_x{k}_{order}"], 3)
    for k in (4, 8):
        out["ratios"][f"composite_k{k}/shade_x{k}"] = round(c[f"composite_k{k}"] / c[f"shade_x{k}"], 3)
    out["ratios"]["layers_k8_shuffled/trace_lds"] = round(c["layers_k8_shuffled"] / c["trace_lds"], 3)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    scene.close()


if __name__ == "__main__":
    main()
