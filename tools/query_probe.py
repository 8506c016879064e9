#!/usr/bin/env python3
"""Point-query throughput against the whole-frame traces of the same rays (run on the GPU box).

    python tools/query_probe.py [--launches 20] [--repeats 5] [--triangles 100000] [--out FILE]

C3 (soup-100k, 1920 x 1080, offsets 0.5) in one process, one scene, one stream. Four cases of
2 073 600 rays each, alternated within every repeat, each timed with device events around
--launches launches after a warm-up launch of each shape:

    query_coherent   the frame's pixel positions in row-major order (rtqQueryAsync)
    query_shuffled   the same positions in a random order
    trace_cull       srtTraceIdsAsync of the frame, cull variant (the tile-cooperative trace)
    trace_lds        srtTraceIdsAsync of the frame, lds variant (brute force)

Reports, per case, Mrays/s and us per launch (median over the repeats) and the spread (min, max).
The sanity condition: both query cases beat trace_lds measured in this very call -- answering
from the lists is the point; trace_cull is context, not a bar. The query answers are also checked
against the cull trace's ids before anything is timed.
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
    ap.add_argument("--launches", type=int, default=20)
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
    pos = {"query_coherent": torch.from_numpy(pos_np).to(dev),
           "query_shuffled": torch.from_numpy(np.ascontiguousarray(pos_np[perm])).to(dev)}
    ids = torch.empty((rays,), dtype=torch.int32, device=dev)
    t = torch.empty((rays,), dtype=torch.float32, device=dev)
    how = torch.empty((rays,), dtype=torch.uint8, device=dev)
    frame = torch.empty((H, W), dtype=torch.int32, device=dev)

    cases = {
        "query_coherent": lambda: scene.query(pos["query_coherent"], ids, t, how, stream=stream),
        "query_shuffled": lambda: scene.query(pos["query_shuffled"], ids, t, how, stream=stream),
        "trace_cull": lambda: scene.trace_ids(off, frame, 0, H, variant="cull", stream=stream),
        "trace_lds": lambda: scene.trace_ids(off, frame, 0, H, variant="lds", stream=stream),
    }
    # Warm-up launch of each shape, and the answers checked while at it.
    cases["trace_cull"]()
    torch.cuda.synchronize()
    want = frame.reshape(-1).clone()
    streamed = {}
    for name in ("query_coherent", "query_shuffled"):
        cases[name]()
        torch.cuda.synchronize()
        expect = want if name == "query_coherent" else want[torch.from_numpy(perm).to(dev)]
        if not torch.equal(ids, expect):
            raise SystemExit(f"{name}: ids differ from the cull trace's")
        streamed[name] = int((how != 0).sum().item())
    cases["trace_lds"]()
    torch.cuda.synchronize()
    if not torch.equal(frame.reshape(-1), want):
        raise SystemExit("trace_lds: ids differ from the cull trace's")

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
    out = {"workload": f"soup-{a.triangles} {W}x{H}, offsets 0.5", "rays_per_launch": rays, "launches": a.launches,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "streamed_queries": streamed, "cases": {}}
    for name, v in us.items():
        med = statistics.median(v)
        out["cases"][name] = {"us_per_launch": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                              "mrays_per_s": round(rays / med, 1)}
        print(json.dumps({name: out["cases"][name]}), flush=True)
    lds = out["cases"]["trace_lds"]["us_per_launch"]
    out["queries_beat_lds"] = all(out["cases"][k]["us_max"] < lds for k in ("query_coherent", "query_shuffled"))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    scene.close()
    if not out["queries_beat_lds"]:
        raise SystemExit("sanity condition failed: a query case is not faster than the lds brute-force trace")


if __name__ == "__main__":
    main()
