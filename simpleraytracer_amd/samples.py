"""Sample offsets for multi-sample frames (include/srt_samples.h; DeviceScene.render_samples) and the
sample tables of the sampled-visibility generators (include/srt_visibility.h; device.Hemisphere,
device.AreaLight)."""
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


def _stratified_unit_square(samples: int, rng) -> np.ndarray:
    """(samples, 2) float64 in [0, 1)^2: sample s jittered inside cell (s % g, s // g) of the
    grid_side(samples) grid."""
    if samples < 1:
        raise ValueError(f"samples must be positive, got {samples}")
    g = grid_side(samples)
    s = np.arange(samples)
    cell = np.stack([s % g, s // g], axis=1).astype(np.float64)
    return (cell + rng.random((samples, 2))) / g


def cosine_hemisphere(samples: int, seed: int) -> np.ndarray:
    """(samples, 3) float32 local directions (lx, ly, lz) around a normal (+z) for device.Hemisphere:
    cosine-weighted -- a stratified point of the unit disc lifted onto the hemisphere --, of unit
    length up to float32 rounding, lz > 0. The seed reproduces the table."""
    u = _stratified_unit_square(samples, np.random.default_rng(seed))
    r, phi = np.sqrt(u[:, 0]), 2.0 * np.pi * u[:, 1]
    d = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u[:, 0])], axis=1)
    out = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    out[:, 2] = np.maximum(out[:, 2], np.float32(2.0 ** -24))  # (lz > 0 after the rounding too)
    return out


def area_samples(samples: int, seed: int) -> np.ndarray:
    """(samples, 2) float32 (a, b) in [0, 1)^2 for device.AreaLight, stratified on the grid_side grid."""
    u = _stratified_unit_square(samples, np.random.default_rng(seed)).astype(np.float32)
    return np.minimum(u, np.nextafter(np.float32(1), np.float32(0)))


def rotations(seed: int) -> np.ndarray:
    """(16, 2) float32 (cos, sin) of 16 uniform angles: device.Hemisphere's per-pixel rotation of its
    sample table, one per pixel of a 4 x 4 block."""
    phi = 2.0 * np.pi * np.random.default_rng(seed).random(16)
    return np.stack([np.cos(phi), np.sin(phi)], axis=1).astype(np.float32)
