"""Sample offsets for multi-sample frames (include/srt_samples.h; DeviceScene.render_samples)."""
from __future__ import annotations

import numpy as np


def grid_side(samples: int) -> int:
    """g of the smallest g x g grid with g * g >= samples."""
    g = 1
    while g * g < samples:
        g += 1
    return g


def stratified_offsets(width: int, height: int, samples: int, seed: int) -> np.ndarray:
    """(samples, H, W, 2) float32 sample offsets: plane s is the frame's offsets of sample s.

    Sample s of every pixel sits in cell s of the smallest g x g grid over the pixel with
    g * g >= samples -- cell (s % g, s // g), row-major -- jittered uniformly inside the cell, so
    the samples of a pixel never bunch. Every value is a float32 in [0, 1) and inside its cell's
    half-open interval [c / g, (c + 1) / g), so positions stay inside their pixel and every tile of
    a frame stays on the traces' in-range path. The seed reproduces the offsets."""
    if samples < 1:
        raise ValueError(f"samples must be positive, got {samples}")
    g = grid_side(samples)
    rng = np.random.default_rng(seed)
    out = np.empty((samples, height, width, 2), np.float32)
    for s in range(samples):  # (plane by plane: the float64 jitter of one plane at a time)
        cell = np.array([s % g, s // g], np.float64)
        plane = ((cell + rng.random((height, width, 2))) / g).astype(np.float32)
        # The rounding to float32 may leave the cell at either end: the smallest float32 >= c / g
        # and the largest < (c + 1) / g bound it.
        lo = (cell / g).astype(np.float32)
        lo = np.where(lo.astype(np.float64) < cell / g, np.nextafter(lo, np.float32(np.inf)), lo)
        hi = np.nextafter(((cell + 1) / g).astype(np.float32), np.float32(-np.inf))
        out[s] = np.clip(plane, lo, hi)
    return out
